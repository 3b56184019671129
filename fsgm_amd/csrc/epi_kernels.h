// epi_kernels.h -- launch interface of the calc_cost_sgm-path kernels: epi_kernels.hip (census, forward-backward check),
// epi_cost.hip, epi_lines.hip + epi_lines_split.hip, epi_wta.hip, epi_sweep.hip, epi_band.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define FSGM_GENERIC_MAX_D 1024

// The disparity ranges of the line kernels and the packed WTA, one row a class: X(D, LPP, DPL) -- LPP adjacent lanes own a pixel,
// DPL consecutive costs each.  16 costs a lane for D = 16 << k; 12, 20 or 28 for the seven ranges between them (144, 176, 208 and
// 240 would take 36 .. 60 costs a lane -- 18 .. 30 state registers and a ring of as many dwords a prefetched step: not offered,
// the generic kernels take them).  agg_line_split, agg_packed_lpp, launch_aggregate and launch_wta are all derived from this list:
// a new class is a new row here.
#define FSGM_LINE_CLASSES(X)                                          \
    X(16, 1, 16) X(32, 2, 16) X(64, 4, 16) X(128, 8, 16) X(256, 16, 16) \
    X(48, 4, 12) X(96, 8, 12) X(192, 16, 12) X(80, 4, 20) X(160, 8, 20) X(112, 4, 28) X(224, 8, 28)
#define FSGM_LINE_CLASS_OK(D, LPP, DPL)                                                                   \
    static_assert((LPP) * (DPL) == (D) && ((LPP) & ((LPP) - 1)) == 0 && (LPP) <= 16 && (DPL) % 4 == 0, \
                  "line class: LPP (a power of two, one DPP row at most) lanes of DPL (whole dwords) costs make up D");
FSGM_LINE_CLASSES(FSGM_LINE_CLASS_OK)
#undef FSGM_LINE_CLASS_OK

namespace fsgm {

struct EpiCostArgs {
    const uint32_t* cen1;   // [frames][NP]
    const uint32_t* cen2;
    const double* pd0;      // [frames][2][NP]
    const double* nd;       // [frames][2][NP]
    const double* off;      // [frames][NP]
    const double* vz;       // [D]  vzInd(d), tabulated on the host with the reference's expression
    double vzmax;           // max |vz[d]| (inf if any is not finite): bounds the sample positions per pixel
    uint8_t* Craw;          // [frames][NP][D]
    int W, H, D;
};

struct AggArgs {
    const uint8_t* C;       // [frames] cost volumes
    uint8_t* L;             // [frames][paths] per-path costs
    size_t c_frame_stride;  // bytes between frames of C
    size_t l_frame_stride;  // bytes between frames of L
    size_t l_dir_stride;    // bytes between path slots of L (= NP*D)
    int W, H, D;
    int P1, P2;
    int ndirs;              // path slots (4 or 8)
    int blk_begin[9];       // first block of each slot, [8] = total
    int dir_code[8];        // bits 1:0 = 0 along x, 1 along y, 2 (+1,+1), 3 (-1,+1); bit 2 = point-mirrored (pass 1)
    // adaptive P2 (calc_cost_sgm.cpp:68-72, adpativeP2 = true): a step uses P2 / 8 where |I1[cur] - I1[pre]| > 25 along the path
    int adaptive = 0;       // line kernels only: 1 selects the ADAPT instantiations
    const uint8_t* I1 = nullptr;   // [frames][NP] the call's first image (read when adaptive)
    size_t i_frame_stride = 0;     // bytes between frames of I1
    // exact path arithmetic (include/fsgm.h, "exact"): no narrowing of a path cost; L then holds y = L_r - C, one byte in [0, P2],
    // per path.  Set by launch_aggregate for AGG_PACKED_EXACT / AGG_GENERIC_EXACT.  Last in the struct, as in WtaArgs
    int exact = 0;
};

struct WtaArgs {
    const uint8_t* L;
    size_t l_frame_stride, l_dir_stride;
    const double* off;      // [frames][NP]
    uint32_t* bestD;        // [frames][NP]
    uint32_t* minC;
    double vMax;
    int W, H, D;
    int ndirs;
    int subpixel, vz_to_disp;
    // runner-up cost (line kernels' WTA only): [frames][NP] min { S[d] : |d - best| >= 2 }, 0xFFFFFFFF where no such d exists;
    // null: not computed.  Last in the struct: every other member keeps its kernarg offset
    uint32_t* minC2;
};
// exact path arithmetic (include/fsgm.h, "exact"): the volumes of WtaArgs::L hold y_r = L_r - C, and the WTA rebuilds
// S = ndirs * C + the sum of the y_r from the frames' cost volumes here.  An argument of its own, after WtaArgs: no kernel that
// takes a WtaArgs sees its arguments move
struct WtaCostArgs {
    const uint8_t* C;       // [frames] cost volumes; null: L holds the path costs themselves
    size_t c_frame_stride;
};

// fused-sweep aggregation (epi_sweep.hip)
struct SweepArgs {
    const uint8_t* C;         // [frames] cost volumes
    size_t c_frame_stride;
    uint8_t* X;               // [frames] u8 sums of a sweep's three y (epi_sweep.hip): written by modes 0/1, read (the other sweep's) by modes 2/3
    size_t x_frame_stride;
    const uint8_t* Lh;        // final modes (2, 3): [frames] the horizontal pair's sum Y_h (pair kernels)
    size_t lh_frame_stride;
    int lh_natural;           // Lh is in natural d order (pairx_* kernels), not the sweeps' private one
    uint2* rec;               // mode 2: [frames][NP] {best | minC << 16, S[best-1] | S[best+1] << 16} (sums of u8 path costs: 16 bits)
    uint16_t* s0;             // mode 2: [frames][NP] S[0] of every pixel
    const uint8_t* state_in;  // [frames][3][W][D] normalised path states of the row above this block
    uint8_t* state_out;       // same, written for the next block
    size_t state_frame_stride;
    int W, H, D;
    int P1, P2;
    int y0, rows;             // rows [y0, y0+rows) of the sweep frame
};

// band sweeps: all four paths of a raster pass in one sweep, one workgroup per frame (epi_band.hip)
struct BandArgs {
    const uint8_t* C;         // [frames] cost volumes
    size_t c_frame_stride;
    uint8_t* Y;               // [frames] low bytes of the first pass's sum of y (private byte order): written by mode 0, read by mode 2
    size_t y_frame_stride;
    uint32_t* Yb;             // [frames][NP][LPP] its 9th bits, one dword per lane (8 paths with 4*P2 > 255), else unused
    size_t yb_frame_stride;   // in dwords
    uint4* edge;              // [frames][W][states][LPP] path states of a band's last row for the band below (3 states at 8 paths, 1 at 4)
    size_t edge_frame_stride; // in uint4
    uint2* rec;               // mode 2: [frames][NP] {best | minC << 16, S[best-1] | S[best+1] << 16} (sums of u8 path costs: 16 bits)
    uint16_t* s0;             // mode 2: [frames][NP] S[0] of every pixel
    uint32_t* Sdbg;           // mode 2, optional: natural-order u32 dump of S [frames][NP][D] (debug tap)
    // chained form: one workgroup per (band, frame), the bands of a frame handing over while they run
    int chain;                // 0: one workgroup per frame, band after band (edge: one map per frame, reused in place)
    uint32_t* ticket;         // work counter, zero at launch
    uint32_t tag;             // 4-bit launch sequence number spread over the top bits of a dword's bytes
    uint32_t* err;            // set to non-zero when a hand-off wait gave up
    int frames, nbands, group; // group: frames whose bands are dealt band-major (tickets)
    int W, H, D;
    int P1, P2;
};

struct SweepSumArgs {          // what wta_sweep_kernel adds up (u8 volumes; the Y volumes in the sweeps' private byte order)
    const uint8_t* C;
    const uint8_t* Xdn;       // Y of the down sweep (or of the vertical pair)
    const uint8_t* Xup;       // Y of the up sweep; may be null
    size_t v_frame_stride;
    const uint8_t* Lh;        // [frames] Y_h of the horizontal pair
    size_t lh_frame_stride;
    int lh_natural;           // Lh is in natural d order (pairx_* kernels), not the private one
    const uint8_t* Lx;        // instead of Lh (then null): [frames][2][N] the two along-x PATH volumes L of the line kernels, natural d order
    size_t lx_frame_stride;
    int nC;                   // S = nC*(C + bias) - (Xdn + Xup + Lh) [+ Lx[0] + Lx[1]: a path's L = (C + bias) - (y + P1)]
    int bias;                 // P2 + P1: the Y volumes hold y + P1 per path (epi_step.h, step_b)
    uint32_t* Sdbg;           // optional natural-order u32 dump of S [frames][NP][D]
};

struct PairArgs {              // an opposite pair of paths as one excess sum (epi_sweep.hip, pair kernels)
    const uint8_t* C;         // [frames] cost volumes
    size_t c_frame_stride;
    uint8_t* X;               // [frames] u8 out: y_fwd + y_bwd (epi_sweep.hip)              (not in the final pass)
    size_t x_frame_stride;
    uint8_t* ckpt;            // [frames][lines][ntiles-1][D] normalised backward states at the tile boundaries
    size_t ckpt_frame_stride;
    const uint8_t* Xother;    // final pass: [frames] the other axis' sum
    size_t xo_frame_stride;
    uint2* rec;               // final pass: [frames][NP] {best | minC << 16, S[best-1] | S[best+1] << 16}
    uint16_t* s0;             // final pass: [frames][NP] S[0] of every pixel
    int nC;                   // final pass: S = nC * (C + P2) - (Y + Yother)
    int xo_natural;           // final pass: Xother is in natural d order (written by the pairx_* kernels), not the private one
    int W, H, D;
    int P1, P2;
};

struct FbArgs {                // forward-backward check (calc_cost_sgm.cpp:429-536)
    const uint32_t* D1;       // [frames][NP] bestD before vz->disparity
    const double* pd0;        // [frames][2][NP]
    const double* nd;         // [frames][2][NP]
    const double* off;        // [frames][NP]
    uint32_t* D2enc;          // [frames][NP] scratch: max(D1 + 1) scattered, 0 = invalid
    uint32_t* D2;             // [frames][NP] out: bestD2 (512<<8 where invalid)
    uint8_t* conf;            // [frames][NP] out: 1 = consistent
    double vMax;
    int W, H, n, thr;
    int linear = 0;           // the reference built without USE_VZIND: the displacement along the direction is D1 / 256 itself (:453, :508)
    int rect = 0;             // +-1: rectified pair -- Pd0 = (x + 1, y + 1), direction (rect, 0) computed in the kernel, pd0 / nd / off not read
    int rect_shift = 0;       // rect * d_min of a search range that starts at d_min: Pd0 = (x + 1 + rect_shift, y + 1)
};

enum { AGG_PACKED_NOWRAP = 0, AGG_PACKED_WRAP = 1, AGG_GENERIC = 2, AGG_SWEEP = 3, AGG_PAIRS = 4, AGG_BAND = 5,
       AGG_PACKED_EXACT = 6, AGG_GENERIC_EXACT = 7 };   // the line kernels without narrowing: P1, P2 in 0..255, any costs

int  agg_packed_lpp(int D);   // lanes per pixel at 16 d per lane -- what the fused pipelines need --, 0 if D is not 16<<k, k<=4
// the general line kernels' and the packed WTA's split of D: lpp lanes of dpl costs a pixel (either may be null).  16 << k as above
// with dpl = 16; 48, 96, 192 (dpl 12), 80, 160 (20), 112, 224 (28); false for every other D: the generic kernels
bool agg_line_split(int D, int* lpp = nullptr, int* dpl = nullptr);
void launch_census(hipStream_t st, const uint8_t* img, uint32_t* cen, int W, int H, int frames);
// The kernels of the cost stage for one frame shape: the one place that decides, for launch_epi_cost, launch_stereo_cost,
// launch_box5x5 and fsgm_epi_cost_kernels (include/fsgm.h).  raw == COST_RAW_FUSED: one kernel, box == COST_BOX_FUSED; every
// other raw kernel writes Craw for one of the three box kernels.  Reads FSGM_COST_FUSED (per call) and FSGM_BOX16 (once).
enum { COST_RAW_FUSED = 0, COST_RAW_PX = 1, COST_RAW_VEC4 = 2, COST_RAW_SCALAR = 3, COST_RAW_STEREO = 4 };
enum { COST_BOX_FUSED = 0, COST_BOX_16 = 1, COST_BOX_4 = 2, COST_BOX_1 = 3 };
struct CostKernels { int raw, box; };
CostKernels select_cost_kernels(int W, int H, int D, bool rectified);
int select_box_kernel(int D);                 // COST_BOX_16 / _4 / _1: the box kernel of a raw volume in HBM
const char* cost_kernels_name(CostKernels k, bool rectified);
void launch_epi_cost(hipStream_t st, const EpiCostArgs& a, uint8_t* C, int frames);
// the cost stage as one kernel (epi_cost.hip): raw costs + 5x5 box mean, a.Craw unused
bool costbox_ok(int W, int H, int D);
void launch_epi_costbox(hipStream_t st, const EpiCostArgs& a, uint8_t* C, int frames);
// the cost stage of a rectified pair (epi_cost.hip): sample cen2[y][clamp(x + direction * d)], direction = -1 / +1; D = 16 << k
// as one kernel, any other D as a raw-cost kernel into Craw and the box kernels.  d_min (|d_min| <= 1024): index d stands for
// disparity d_min + d, the sample is cen2[y][clamp(x + direction * (d_min + d))]
void launch_stereo_cost(hipStream_t st, const uint32_t* cen1, const uint32_t* cen2, uint8_t* Craw, uint8_t* C, int W, int H, int D,
                        int direction, int frames, int d_min = 0);
// disp (and disp2 unless null) of n pixels in place as int32 true disparities: 256 * d_min + value, disp2's 512 << 8 -> INT32_MIN
void launch_stereo_range(hipStream_t st, uint32_t* disp, uint32_t* disp2, size_t n, int d_min);
void launch_box5x5(hipStream_t st, int box, const uint8_t* Craw, uint8_t* C, int W, int H, int D, int frames);   // box: select_box_kernel(D)
int  costbox_selftest(hipStream_t st);      // 0: the mean's fp16 multiply is exact on this device; > 0: mismatches; < 0: could not run
void launch_aggregate(hipStream_t st, AggArgs a, int paths, int frames, int kernel_kind);
// x.C set: an exact plan's volumes (never with a.minC2: the plan refuses the pair)
void launch_wta(hipStream_t st, const WtaArgs& a, int frames, bool packed, WtaCostArgs x = WtaCostArgs{nullptr, 0});
int    sweep_rows_per_launch(int D);
size_t sweep_state_bytes(int W, int D);   // one state buffer of one frame
void launch_sweep(hipStream_t st, const SweepArgs& a, int frames, int mode, int tall = 0);
// rows [ybeg, yend) of the sweep frame; modes 2 / 3: final on the mirrored / the pass-0 frame; *parity carries the state buffer in use from one range of a sweep to the next
void launch_sweep_rows(hipStream_t st, const SweepArgs& a, int frames, int mode, int tall, int ybeg, int yend, int* parity);   // 0 down, 1 up, 2 up + fused WTA; tall: 8-wave workgroups (modes 0, 1)
size_t pair_ckpt_bytes(int W, int H, int D, int axis);      // per frame; axis 0 horizontal, 1 vertical
void launch_pair(hipStream_t st, const PairArgs& a, int frames, int axis, bool final_pass, int phase = 0);
bool pair_x_fine_ok(int D);                                                        // the along-x pair with 8 costs a lane exists for this D
void launch_pair_x_fine(hipStream_t st, const PairArgs& a, int frames);            // checkpoint + sum pass, Y in natural d order
size_t band_edge_uint4s(int W, int D, int paths);           // one hand-off map between two bands of one frame, in uint4
int    band_rows(int D);                                    // rows per band
size_t band_bits_u32s(int W, int H, int D);                 // bit plane of one frame, in dwords
bool   band_needs_bits(int paths, int P1, int P2);
bool   band_ok(int D, int paths, int P1, int P2, int cmax);
void launch_band(hipStream_t st, const BandArgs& a, int frames, int paths, int mode);   // 0 first pass, 2 second pass + WTA records
void launch_sweep_finish(hipStream_t st, const WtaArgs& a, const uint2* rec, const uint16_t* s0, int frames);
void launch_wta_sweep(hipStream_t st, const WtaArgs& a, const SweepSumArgs& q, int frames);
void launch_fb_check(hipStream_t st, const FbArgs& a, int frames);
void launch_vz_convert(hipStream_t st, uint32_t* bestD, const double* off, int W, int H, int D, double vMax, int frames);
int  fused_step_selftest(hipStream_t st);   // 0: pk_max3 / pk_min3 of the fused step are exact u16 operations here
void launch_copy16(hipStream_t st, void* dst, const void* src, size_t bytes);   // bytes % 4096 == 0; bandwidth probe
void launch_sum_paths(hipStream_t st, const uint8_t* L, uint32_t* S, size_t n, size_t dir_stride, int ndirs);
// the same over an exact plan's volumes: S = ndirs * C + the sum of the y_r in L
void launch_sum_paths_exact(hipStream_t st, const uint8_t* L, const uint8_t* C, uint32_t* S, size_t n, size_t dir_stride, int ndirs);

}  // namespace fsgm
