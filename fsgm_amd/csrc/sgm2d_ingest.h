// sgm2d_ingest.h -- caller-supplied 2-D cost volumes, already in HBM, into a fsgm_pyd_plan's C: u8 [n][H][W][PS], a pixel's
// candidate (sx, sy) at sx*RS + sy with RS = pyd_row_stride(Sx, Sy), PS = Sx*RS (pyd_kernels.h), the RS - Sy padding bytes
// of every row written as 0.  Three source layouts (include/fsgm.h, FSGM_COST2D_LAYOUT_*): the reference's [H][W][Sx*Sy],
// and the two channel-major orders of a torch (N, D, H, W) tensor, transposed through an LDS tile.  Every byte is saturated
// at the caller's declared bound and a device flag is raised when one was above it, as sgm_ingest.h does for the 1-D
// matcher's volumes; its byte tricks and its tile are used here.  Kernels: sgm2d_ingest.hip.
#pragma once
#include "sgm_ingest.h"

namespace fsgm {

// n volumes from src (any byte alignment) into dst (16-byte aligned, n * W*H*PS bytes), every byte min(byte, bound), padding
// 0; *flag = 1 (flag may be NULL) when some byte was above the bound.  bound 1..255; Sx, Sy the window's sides.
void launch_sgm2d_ingest(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int W, int H, int Sx, int Sy, int layout, int bound,
                         uint32_t* flag);
// the LDS the launcher asks for (static, per workgroup): nothing for FSGM_COST2D_LAYOUT_HWD, one tile for the other two
size_t sgm2d_ingest_lds_bytes(int layout);

}  // namespace fsgm
