// epi_view2.h -- launch interface of epi_view2.hip: the second-view disparity from the line kernels' path volumes (include/fsgm.h,
// "Second view"), and the left-right check on a pair of disparity maps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace fsgm {

// The second view's winner-take-all over the diagonal of S = the sum of the path volumes: for second-view pixel (x2, y) the
// candidates are the i in [0, D) whose first-view pixel x = x2 - dir * (d_min + i) lies in [0, W).
struct View2Args {
    const uint8_t* L;       // [frames][ndirs] path volumes of the line kernels (WtaArgs::L)
    size_t l_frame_stride, l_dir_stride;
    const uint8_t* C;       // an exact plan's cost volumes (the volumes hold L_r - C: S = ndirs * C + their sum); null otherwise
    size_t c_frame_stride;
    uint32_t* disp2;        // [frames][NP] out: index * 256 (+ parabola) + add, `marker` where no candidate exists
    uint32_t* minC2v;       // [frames][NP] out, may be null: S at the winner, all ones where no candidate exists
    int W, H, D, ndirs;
    int dir, d_min;         // dir -1 / +1
    int subpixel;
    uint32_t add, marker;   // the sgm(C) forms: 0 and all ones; the stereo forms: 256 * d_min and INT32_MIN
};

// The left-right check, one thread a pixel: with d1 = (((int32)disp[p] - pre1) << shift1) + add1 (shift1 = 8, pre1 = the shift the
// map carries: a call without sub-pixel returns whole candidate indices in its first view; otherwise 0 and 0), x2 = x + dir * ((d1 + 128) >> 8) and
// d2 = (int32)disp2[y][x2] + add2: conf = 0 <= x2 < W and disp2[y][x2] != marker2 and |d1 - d2| <= max_diff (int64)
struct View2CheckArgs {
    const uint32_t* disp;   // [frames][NP]
    const uint32_t* disp2;  // [frames][NP]
    uint8_t* conf;          // [frames][NP] out
    int W, H, dir, max_diff;
    int32_t add1, add2, pre1, shift1;
    uint32_t marker2;
};

int    view2_tile(int D);           // second-view pixels a workgroup of the tiled kernel owns (D <= 256), 0: the generic kernel
size_t view2_lds_bytes(int D);      // dynamic LDS the launcher asks for, per workgroup
void launch_view2(hipStream_t st, const View2Args& a, int frames);
void launch_view2_check(hipStream_t st, const View2CheckArgs& a, int frames);

}  // namespace fsgm
