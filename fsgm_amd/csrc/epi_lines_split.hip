// epi_lines_split.hip -- the line aggregation at D = 48 .. 224: the classes of FSGM_LINE_CLASSES (epi_kernels.h) with 12, 20 or
// 28 costs a lane.  A unit of its own so that neither half of the line kernels is the build's longest compile.
#include "epi_lines.h"

namespace fsgm {

// D = 48 .. 224 (agg_line_split: LPP x DPL with DPL = 12, 20 or 28): the general body for every direction with that one split
// -- no finer split along x, none of the hand-written steps, whose register layouts are 2 or 16 costs a lane
template <int D, int DPL, bool WRAP, bool ADAPT>
__global__ __launch_bounds__(256) void agg_split_kernel(AggArgs a) {
    int slot = 0;                       // which direction slot does this block belong to (block-uniform)
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const bool mirror = (code & 4) != 0;
    switch (code & 3) {                 // 0: along x, 1: along y, 2: x+1,y+1, 3: x-1,y+1
        case 0: agg_packed_body<D, DPL, WRAP, 0, ADAPT>(a, slot, mirror); break;
        case 1: agg_packed_body<D, DPL, WRAP, 1, ADAPT>(a, slot, mirror); break;
        case 2: agg_packed_body<D, DPL, WRAP, 2, ADAPT>(a, slot, mirror); break;
        default: agg_packed_body<D, DPL, WRAP, 3, ADAPT>(a, slot, mirror); break;
    }
}

// the same with exact path arithmetic (epi_lines.h, EXACT): kernels of their own, so that the ones above stay what they were
template <int D, int DPL, bool ADAPT>
__global__ __launch_bounds__(256) void agg_split_exact_kernel(AggArgs a) {
    int slot = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const bool mirror = (code & 4) != 0;
    switch (code & 3) {
        case 0: agg_packed_body<D, DPL, false, 0, ADAPT, true>(a, slot, mirror); break;
        case 1: agg_packed_body<D, DPL, false, 1, ADAPT, true>(a, slot, mirror); break;
        case 2: agg_packed_body<D, DPL, false, 2, ADAPT, true>(a, slot, mirror); break;
        default: agg_packed_body<D, DPL, false, 3, ADAPT, true>(a, slot, mirror); break;
    }
}

template <int D, int DPL>
static void launch_split(hipStream_t st, AggArgs& a, int paths, int frames, bool wrap) {
    if constexpr (DPL != 16) {                                   // (16 costs a lane: launch_packed, epi_lines.hip)
        constexpr int LPB = 4 * (64 / (D / DPL));                // lines per block, every direction
        plan_dirs(a, paths, LPB, LPB);
        dim3 grid(a.blk_begin[8], frames);
        if (a.exact) {
            if (a.adaptive) hipLaunchKernelGGL((agg_split_exact_kernel<D, DPL, true>), grid, dim3(256), 0, st, a);
            else            hipLaunchKernelGGL((agg_split_exact_kernel<D, DPL, false>), grid, dim3(256), 0, st, a);
        } else if (a.adaptive) {
            if (wrap) hipLaunchKernelGGL((agg_split_kernel<D, DPL, true, true>), grid, dim3(256), 0, st, a);
            else      hipLaunchKernelGGL((agg_split_kernel<D, DPL, false, true>), grid, dim3(256), 0, st, a);
        } else {
            if (wrap) hipLaunchKernelGGL((agg_split_kernel<D, DPL, true, false>), grid, dim3(256), 0, st, a);
            else      hipLaunchKernelGGL((agg_split_kernel<D, DPL, false, false>), grid, dim3(256), 0, st, a);
        }
    }
}

void launch_split_lines(hipStream_t st, AggArgs& a, int paths, int frames, bool wrap) {
    switch (a.D) {
#define FSGM_X(D, LPP, DPL) case D: launch_split<D, DPL>(st, a, paths, frames, wrap); break;
        FSGM_LINE_CLASSES(FSGM_X)
#undef FSGM_X
        default: break;
    }
}

}  // namespace fsgm
