/*
 * fsgm.h -- C ABI of libfsgm_hip.so: fSGM's matching-cost + multi-path SGM hot path on
 * AMD Instinct MI355X (gfx950, hand-written HIP).
 *
 * This is the drop-in boundary.  Every entry point below replaces one function of the
 * reference's MEX layer (file:line cited per function, relative to the fSGM tree).  The four
 * mexFunction gateways in fsgm_amd/mex/ are thin shims over the *_host entry points: host
 * pointers in, host pointers out, plain C types only, nothing of torch/HIP in a signature
 * (streams travel as void*).
 *
 * Memory order is the reference's native order, i.e. what MATLAB hands a MEX after the
 * drivers' permute([2 1 3]) (epipolar_sgm_of.m:33-43, pyramidal_sgm.m:44-46, ng_sgm.m:15-17):
 *   images  u8  [height][width]        x fastest      (MATLAB: width x height, column-major)
 *   maps    f64 [plane][height][width] plane 0 = x    (MATLAB: width x height x 2)
 *   volumes u8  [height][width][D]     d fastest      (calc_cost_sgm.cpp:345,389)
 *
 * There is NO CPU fallback in this library: every compute entry point needs a HIP device and
 * fails with FSGM_ERR_HIP when there is none.
 */
#ifndef FSGM_H
#define FSGM_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FSGM_VERSION_MAJOR 0
#define FSGM_VERSION_MINOR 1

typedef enum {
    FSGM_OK = 0,
    FSGM_ERR_INVALID = 1,      /* bad argument (null pointer, size, class) -- the reference validates nothing */
    FSGM_ERR_HIP = 2,          /* HIP runtime error / no device */
    FSGM_ERR_NOMEM = 3,
    FSGM_ERR_UNSUPPORTED = 4
} fsgm_status;

/* Thread-local text of the last error returned on this thread. */
const char* fsgm_last_error(void);
/* Number of HIP devices visible (0 if none / no runtime). */
int fsgm_device_count(void);
/* "gfx950"-style arch string of a device, written into buf. */
fsgm_status fsgm_device_arch(int device, char* buf, size_t buflen);
/* Free every cached plan / HBM buffer held for the *_host entry points (mexAtExit hook). */
void fsgm_shutdown(void);

/* ------------------------------------------------------------------------------------------
 * calc_cost_sgm  (calc_cost_sgm.cpp:539-598, called from epipolar_sgm_of.m:45)
 * ------------------------------------------------------------------------------------------ */

/* Run-time form of the reference's compile-time switches.  fsgm_epi_params_default() returns
 * the shipped values. */
typedef struct {
    int32_t paths;        /* 4 = as shipped (enableDiagnalPath=false, calc_cost_sgm.cpp:104); 8 = with diagonals */
    int32_t subpixel;     /* 1 = as shipped (subPixelRefine=true, calc_cost_sgm.cpp:560) */
    int32_t vz_to_disp;   /* 1 = as shipped (USE_VZIND, calc_cost_sgm.cpp:4,592-594) */
    int32_t device;       /* HIP device ordinal */
    int32_t fb_check;     /* 0 = as shipped (call commented out, calc_cost_sgm.cpp:589-590: conf and bestD2 stay 0);
                             1 = run forward_backward_check (:482-536, threshold 2) on bestD before vz->disparity.
                             Needs dMax <= 511 (bestD must stay below INVALID_DISPARITY = 512<<8) */
} fsgm_epi_params;

fsgm_epi_params fsgm_epi_params_default(void);

typedef struct {
    const uint8_t* I1;            /* prhs[0]  u8 [H][W] */
    const uint8_t* I2;            /* prhs[1] */
    int32_t width, height;        /* mxGetM / mxGetN of prhs[0] (calc_cost_sgm.cpp:562-563) */
    int32_t dMax;                 /* prhs[2] */
    double  vMax;                 /* prhs[3] */
    const double* pixelPosD0;     /* prhs[4]  f64 [2][H][W], 1-based coordinates */
    const double* normDir;        /* prhs[5]  f64 [2][H][W] */
    const double* offset;         /* prhs[6]  f64 [H][W] */
    int32_t P1, P2;               /* prhs[7], prhs[8] (truncated to int like mxGetScalar -> int) */
} fsgm_epi_in;

typedef struct {
    uint32_t* bestD;              /* plhs[0]  u32 [H][W], disparity * 256 */
    uint32_t* minC;               /* plhs[1]  u32 [H][W] */
    /* optional debug taps (NULL = not wanted): the cost volume C (u8 [H][W][D]) and the summed
     * path costs S (u32 [H][W][D]) -- internal arrays of the reference (calc_cost_sgm.cpp:579,95) */
    uint8_t*  C;
    uint32_t* S;
    /* plhs[2], plhs[3]: filled only when fb_check = 1 and the pointer is not NULL (the caller's
     * zero-initialised arrays stay untouched otherwise, like in the shipped reference) */
    uint8_t*  conf;               /* u8  [H][W], 1 = forward-backward consistent */
    uint32_t* bestD2;             /* u32 [H][W], disparity of the second view, 512<<8 where invalid */
} fsgm_epi_out;

/* One frame, host pointers in / host pointers out.  This is what the calc_cost_sgm gateway
 * calls. */
fsgm_status fsgm_calc_cost_sgm_host(const fsgm_epi_in* in, const fsgm_epi_out* out,
                                    const fsgm_epi_params* prm);

/* A batch of independent frames of identical shape, processed concurrently on one device. */
fsgm_status fsgm_calc_cost_sgm_batch_host(int32_t n_frames, const fsgm_epi_in* in,
                                          const fsgm_epi_out* out, const fsgm_epi_params* prm);

/* calc_cost_sgm as the reference builds it WITHOUT line 4 (#define USE_VZIND): a plain 1-D matcher along an arbitrary direction
 * field.  Candidate d is sampled d pixels along the per-pixel direction,
 *   x2 = clamp((int)round((Pd0x - 1) + d * ux), 0, W - 1), likewise y                     (calc_cost_sgm.cpp:368-375),
 * no vz -> disparity conversion runs (:592-594: bestD is the index * 256, truncating) and the forward-backward check works on
 * bestD / 256 directly (:452-453, :507-508).  Same structs as the vz-index entry points: in->vMax and in->offset are accepted
 * and ignored (offset may be NULL), prm->vz_to_disp is ignored; paths, subpixel, device and fb_check are honoured
 * (fb_check = 1 needs dMax <= 511).  Box mean, aggregation, WTA and parabola are those of fsgm_calc_cost_sgm_host. */
fsgm_status fsgm_calc_cost_sgm_linear_host(const fsgm_epi_in* in, const fsgm_epi_out* out,
                                           const fsgm_epi_params* prm);
fsgm_status fsgm_calc_cost_sgm_linear_batch_host(int32_t n_frames, const fsgm_epi_in* in,
                                                 const fsgm_epi_out* out, const fsgm_epi_params* prm);

/* Options beyond fsgm_epi_params / fsgm_stereo_params, which keep their size: the *_opts entry points below and further down take
 * one of these (NULL = the defaults, all zero) next to the parameter struct of the entry point they extend, and compute
 * exactly what that entry point computes when every option is off -- the older entry points forward to them with NULL.
 *   adaptive_p2: 0 = as shipped (`const bool adpativeP2 = false`, calc_cost_sgm.cpp:102); 1 = the reference's edge-aware large
 *   penalty (adaptive_P2, :68-72): every step of every path uses P2cur = |I1[cur] - I1[pre]| > 25 ? P2 / 8 : P2 in place of
 *   P2, the division C's truncating int division, cur the pixel being computed, pre its predecessor on that path, I1 the call's
 *   first image (all three samplings).  Path starts take no step.  Everything downstream is unchanged.  Adaptive calls
 *   aggregate with the per-direction line kernels at every batch size (aggregation mode 1); the exact / mod-256 choice is
 *   still made with the full P2.
 * `reserved` must be zero. */
typedef struct {
    int32_t adaptive_p2;
    int32_t reserved[7];
} fsgm_epi_options;

fsgm_epi_options fsgm_epi_options_default(void);       /* all zero */

fsgm_status fsgm_calc_cost_sgm_host_opts(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                         const fsgm_epi_options* opt);
fsgm_status fsgm_calc_cost_sgm_batch_host_opts(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                               const fsgm_epi_params* prm, const fsgm_epi_options* opt);
fsgm_status fsgm_calc_cost_sgm_linear_host_opts(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                                const fsgm_epi_options* opt);
fsgm_status fsgm_calc_cost_sgm_linear_batch_host_opts(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                                      const fsgm_epi_params* prm, const fsgm_epi_options* opt);

/* ------------------------------------------------------------------------------------------
 * Rectified stereo: a left/right pair in, a disparity map out.  The linear matcher above with Pd0 = (x + 1, y + 1) and
 * direction (direction, 0) -- the sample of candidate d is cen2[y][clamp(x + direction * d, 0, W - 1)] -- without any map:
 * the cost stage is a kernel of its own and only the two images are uploaded.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t paths;        /* 4 or 8, as fsgm_epi_params */
    int32_t subpixel;     /* 1 = parabola refinement (disparity in 1/256 steps), 0 = whole disparities * 256 */
    int32_t fb_check;     /* 1 = the reference's forward-backward check (calc_cost_sgm.cpp:429-536, threshold 2): conf, disp2; dMax <= 511 */
    int32_t direction;    /* -1: I1 is the left view, the match in I2 lies at x - d; +1: the match lies at x + d */
    int32_t device;       /* HIP device ordinal */
} fsgm_stereo_params;

fsgm_stereo_params fsgm_stereo_params_default(void);   /* 4, 1, 0, -1, 0 */

/* n_frames contiguous pairs I1 / I2 u8 [n][H][W] -> disp u32 [n][H][W] (disparity * 256) and minC u32 [n][H][W]; with
 * fb_check = 1 also conf u8 [n][H][W] (1 = consistent) and disp2 u32 [n][H][W] (second view, 512<<8 where invalid), each of
 * which may be NULL; without fb_check they are not written.  prm may be NULL (the defaults).  Aggregation pipelines are
 * selected as for fsgm_calc_cost_sgm_batch_host. */
fsgm_status fsgm_stereo_sgm_host(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                 int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp,
                                 uint32_t* minC, uint8_t* conf, uint32_t* disp2);
/* the same with options (fsgm_epi_options above: adaptive_p2 reads I1, the left view when direction = -1) */
fsgm_status fsgm_stereo_sgm_host_opts(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                      int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                      const fsgm_epi_options* opt, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2);

/* A search range that starts at d_min instead of 0: candidate index i in [0, dMax) stands for disparity d_min + i, sampled at
 * cen2[y][clamp(x + direction * (d_min + i), 0, W - 1)] -- the linear matcher on Pd0 = (x + 1 + direction * d_min, y + 1),
 * direction (direction, 0), which is also what the forward-backward check works on.  d_min may be negative (converged or
 * shifted principal points); |d_min| <= FSGM_D_MIN_LIMIT, anything else is FSGM_ERR_INVALID before a device is touched.
 * Arguments as fsgm_stereo_sgm_host_opts plus d_min; the outputs that carry disparities are int32 TRUE disparities * 256:
 *   disp  = 256 * d_min + (index * 256 + parabola offset)
 *   disp2 = the same for the second view, INT32_MIN where invalid (512 << 8, the marker of the entry points above, is a valid
 *           value once d_min > 0)
 * minC and conf are as above.  d_min = 0 gives the values of fsgm_stereo_sgm_host_opts read as int32, with INT32_MIN for
 * disp2's marker.  Aggregation, WTA and pipeline selection are those of the same dMax without d_min.
 * The cached plan is shared by every d_min of a shape: the key does not hold it; each stereo entry point -- these and the ones
 * above, which set 0 -- sets the plan's shift under the plan's lock before it queues anything, so no call sees another's. */
#define FSGM_D_MIN_LIMIT 1024
fsgm_status fsgm_stereo_sgm_host_range(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                       int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                       const fsgm_epi_options* opt, int32_t d_min, int32_t* disp, uint32_t* minC, uint8_t* conf,
                                       int32_t* disp2);

/* The runner-up cost: how unambiguous the winner-take-all's choice was.  With S[d], d in [0, dMax), the u32 sums of the path
 * volumes (fsgm_epi_plan_download_sum), best the WTA's index -- the first strict minimum, before the parabola, the vz
 * conversion and d_min -- and minC = S[best]:
 *   minC2 = min { S[d] : |d - best| >= 2 },  FSGM_NO_RUNNER_UP where no such d exists (dMax <= 2; dMax = 3 with best = 1).
 * It belongs to the first view's WTA and depends on none of subpixel, vz_to_disp, fb_check, d_min, direction.  Only the WTA of
 * the line kernels writes it: a plan or a call that asks for it runs "packed16/nowrap", "packed16/wrap" or "generic" at every
 * batch size (fsgm_epi_plan_set_runner_up below).
 * fsgm_stereo_sgm_host_ru: fsgm_stereo_sgm_host_range with minC2 u32 [n][H][W] after minC; minC2 must not be NULL.  Its cached
 * plan is never the one of a call without minC2: those keep their pipelines and their outputs. */
#define FSGM_NO_RUNNER_UP 0xFFFFFFFFu
/* The pipeline the calling thread's last successful fsgm_stereo_sgm_* call ran, host or device form ("" before the first), in
 * the names of fsgm_epi_plan_kernel_name: how a caller sees that a call with minC2 ran the line kernels and one without kept
 * its fused pipeline. */
const char* fsgm_stereo_sgm_last_kernel(void);
fsgm_status fsgm_stereo_sgm_host_ru(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                    int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                    const fsgm_epi_options* opt, int32_t d_min, int32_t* disp, uint32_t* minC, uint32_t* minC2,
                                    uint8_t* conf, int32_t* disp2);
/* The uniqueness test (OpenCV's uniquenessRatio) on such a pair of costs: out = NaN where
 *   minC2 != FSGM_NO_RUNNER_UP  and  (u64)minC2 * (100 - ratio) < (u64)minC * 100,
 * map elsewhere (NaN stays NaN).  map, out f64 and minC, minC2 u32, [n][H][W] each; ratio in [0, 100], 0 rejects nothing.  A
 * ratio outside that range, a NULL pointer or a size below 1 is FSGM_ERR_INVALID before a device is touched.  out may be map
 * itself; it may not overlap map otherwise, nor minC or minC2 (FSGM_ERR_INVALID).  The device form follows the device-pointer
 * contract below; its status word is always 0. */
fsgm_status fsgm_uniqueness_filter_host(int32_t n_frames, const double* map, const uint32_t* minC, const uint32_t* minC2,
                                        int32_t width, int32_t height, int32_t ratio, double* out, int32_t device);
fsgm_status fsgm_uniqueness_filter_device(int32_t n_frames, const double* map, const uint32_t* minC, const uint32_t* minC2,
                                          int32_t width, int32_t height, int32_t ratio, double* out, int32_t device, void* stream,
                                          int32_t* status);
/* The runner-up cost of the 2-D matcher (calc_pyd_cost_sgm, sgm2d(C), the fsgm_pyd_plan).  For one pixel let S[sx*Sy + sy] be the
 * u32 sums its WTA minimises -- exactly what the S tap returns, wrapping penalties included -- and best = bx*Sy + by the WTA's
 * index, the first strict minimum in candidate order:
 *   minC2 = min { S[sx*Sy + sy] : max(|sx - bx|, |sy - by|) >= 2 },  FSGM_NO_RUNNER_UP where that set is empty.
 * The set is empty for every window with both sides <= 2, and for a side of 3 with the best in its middle while the other side
 * is <= 3.  The excluded ring is the eight candidates the x and y parabolas and their diagonals draw on: the same minimum, not
 * a competitor.  With Sy == 1 the rule is the 1-D rule |d - best| >= 2 above.  bestD, minC, mvSub, flow and S of a call that
 * asks for minC2 are bit-identical to those of the same call without it; the cost and aggregation kernels are the same.
 * Entry points: fsgm_pyd_plan_set_runner_up / _download_runner_up, fsgm_calc_pyd_cost_sgm_batch_host_ru,
 * fsgm_sgm2d_batch_host_ru / fsgm_sgm2d_device_ru, fsgm_sgm2d_batch_host_exact / fsgm_sgm2d_device_exact (minC2 non-NULL; S then
 * the exact sums); on 1-D volumes fsgm_sgm_batch_host_ru / fsgm_sgm_device_ru (the 1-D rule).
 *
 * The uniqueness test above on `planes` planes per frame: planes = 1 is fsgm_uniqueness_filter_host itself, planes = 2 takes a
 * flow -- map, out f64 [n][2][H][W], minC, minC2 u32 [n][H][W] -- and writes NaN into both planes of a rejected pixel.  planes
 * outside 1..2 is FSGM_ERR_INVALID before a device is touched; the overlap rules are the ones above on the arrays' full sizes. */
fsgm_status fsgm_uniqueness_filter_planes_host(int32_t n_frames, const double* map, const uint32_t* minC, const uint32_t* minC2,
                                               int32_t width, int32_t height, int32_t planes, int32_t ratio, double* out,
                                               int32_t device);
fsgm_status fsgm_uniqueness_filter_planes_device(int32_t n_frames, const double* map, const uint32_t* minC, const uint32_t* minC2,
                                                 int32_t width, int32_t height, int32_t planes, int32_t ratio, double* out,
                                                 int32_t device, void* stream, int32_t* status);
/* The runner-up cost of the neighbour-guided matcher (calc_pyd_cost_sgm_ng, the level of fsgm_pyramidal_sgm_ng).  A pixel has
 * D = 9 (2r+1)^2 candidates, each with an integer motion vector (mvx_d, mvy_d) and a u32 sum S[d] -- what the S tap returns.  The
 * winner is the first minimum of S over d, as without the switch; let (bx, by) be its vector:
 *   minC2 = min { S[d] : max(|mvx_d - bx|, |mvy_d - by|) >= 2 },  FSGM_NO_RUNNER_UP where that set is empty.
 * The distance is between motion vectors, not list indices (the differences are exact for every int32 vector): the same
 * "Chebyshev distance >= 2" as the 2-D rule.  Repeats of the winner's vector -- the nine neighbours' hints overlap, so lists are
 * full of them -- are never runners-up, whatever their sums.  The consequence: where all nine neighbours' hints (those of
 * (x +- 8, y +- 8), clamped to the map) agree on h, every candidate lies within distance 1 of h when r <= 1.  With r = 0, or
 * with r = 1 and h itself the winner, no runner-up exists and the uniqueness test keeps the pixel: the matcher considered one
 * hypothesis there, which says nothing against it.  With r = 1 and a winner on the ring around h, the ring's other side is two
 * away and competes, by the rule as it stands.
 * minC, flow and S of a call that asks for minC2 are bit-identical to those of the same call without it, with and without
 * subPixelRefine; minC2 does not depend on subPixelRefine.
 * Entry points: fsgm_calc_pyd_cost_sgm_ng_host_ru / _batch_host_ru; for level 1 of the pyramids (both matchers, each by its
 * own rule) fsgm_pyramidal_sgm_host_ru / _device_ru, fsgm_pyramidal_sgm_ng_host_ru / _device_ru, fsgm_pyramid_plan_set_runner_up
 * / _download_runner_up and the same pair of fsgm_ng_pyramid_plan_*; with the filter fsgm_pyramidal_flow_pp_host_u / _device_u. */

/* ---- device-resident plan: buffers for `batch` frames stay in HBM across calls ---- */
typedef struct fsgm_epi_plan fsgm_epi_plan;

/* stage bits for fsgm_epi_plan_run / _time */
#define FSGM_STAGE_COST      1   /* census x2 + Hamming cost fill + 5x5 box   (calc_cost_sgm.cpp:319-412) */
#define FSGM_STAGE_AGGREGATE 2   /* multi-path DP: C -> per-path L_r          (calc_cost_sgm.cpp:86-257)  */
#define FSGM_STAGE_WTA       4   /* sum of paths, argmin, parabola, vz->disp  (calc_cost_sgm.cpp:259-308,414-426) */
#define FSGM_STAGE_ALL       7

fsgm_status fsgm_epi_plan_create(fsgm_epi_plan** plan, int32_t width, int32_t height,
                                 int32_t dMax, int32_t batch, const fsgm_epi_params* prm);
/* How a plan samples candidate d, fixed at creation.  fsgm_epi_plan_create makes FSGM_SAMPLING_VZ plans. */
#define FSGM_SAMPLING_VZ        0   /* offset * vzInd(d) along the direction: the reference as shipped (USE_VZIND) */
#define FSGM_SAMPLING_LINEAR    1   /* d pixels along the direction: the reference without USE_VZIND; the offset map is unused
                                       (fsgm_epi_plan_upload accepts NULL for it), vz_to_disp is off */
#define FSGM_SAMPLING_RECTIFIED 2   /* rectified pair: Pd0 = (x + 1, y + 1), direction (direction, 0), direction = -1 or +1.  The plan
                                       never allocates coordinate or offset maps and takes images only
                                       (fsgm_epi_plan_upload_images); its FSGM_STAGE_COST is the rectified cost kernel */
fsgm_status fsgm_epi_plan_create_sampling(fsgm_epi_plan** plan, int32_t width, int32_t height, int32_t dMax, int32_t batch,
                                          const fsgm_epi_params* prm, int32_t sampling, int32_t direction);
void        fsgm_epi_plan_destroy(fsgm_epi_plan* plan);
fsgm_status fsgm_epi_plan_set_penalties(fsgm_epi_plan* plan, int32_t P1, int32_t P2, double vMax);
/* Aggregation strategy: 0 = auto, 1 = the per-direction line kernels, 2 = the fused pipeline whenever eligible
 * (8 paths: horizontal pair + down sweep + final up sweep with the WTA inside -- D = 16<<k, no-wrap penalties with
 * P1 <= P2 and 3*(P1+P2) <= 255; the shipped 4 paths: the pair kernels -- 2*(P1+P2) <= 255), 3 = 8 paths only: the down and the
 * up sweep side by side and a WTA kernel over the three sums (half the latency of 2, 3 B per voxel more traffic),
 * 4 = the band sweeps (epi_band.hip: all four paths of a raster pass in one sweep, one workgroup per frame, for batches of
 * hundreds of frames; D = 16<<k, no-wrap penalties with P1 <= P2, P1 + P2 <= 127), 5 = the band sweeps with the bands of a
 * frame as workgroups of their own that hand their last row over while they run ("band16chain/nowrap"),
 * 6 = 8 paths only: as 3, but the two sweeps meet in the middle -- each writes its sum for its first half of the rows and crosses
 * the other's half as a final sweep with the WTA inside ("sweep16mid/nowrap": the traffic of 2 on the chain of 3).
 * Auto picks by batch size, frame shape and path count; fsgm_epi_auto_pipeline() below answers for any configuration and
 * fsgm_epi_plan_kernel_name() for a plan.  At 1242x375x128, 256 CUs: 8 paths -- line kernels below 4 frames, 3 below 10, 6 below 26,
 * 2 up to ~229, then 4 where a round of one workgroup per frame pays (230-256, 473-512, ...) and 5 between those rounds; 4 paths --
 * line kernels below 9 frames, then 2, then 4 / 5 likewise.  The switch points move with the frame shape by voxels^(-2/3)
 * (FSGM_EPI_SHAPE_SCALE).  Results are identical in every mode.  Modes 2-6 leave the line kernels in place where they do
 * not apply: wrapping penalties, and every dMax other than 16, 32, 64, 128, 256 (fsgm_epi_plan_kernel_name below).
 * HBM a plan holds per frame beyond C (allocated when a mode first runs, kept until the plan is destroyed; N = W*H*D bytes):
 * mode 1: paths x N (path volumes); mode 2: 2 N + N/8 + boundary states (8 paths) / N + 2 N/8 (4 paths); modes 3, 6: one more N;
 * modes 4, 5: N + N/4 (9th-bit plane, 8 paths only) + one hand-off map of 3*W*D bytes (mode 5: one per band boundary,
 * ~1.4 B per voxel at 1242x375x128), + 10 bytes per pixel of WTA records for modes 2-5.  Mode 5 synchronises its
 * workgroups through bounded polls on device memory; a poll that gives up raises a flag that fsgm_epi_plan_sync / _download /
 * _time report as FSGM_ERR_HIP.  The cost stage's own buffers (images, census, coordinate maps) appear with the first upload
 * or FSGM_STAGE_COST run: an aggregation-only plan never allocates them. */
fsgm_status fsgm_epi_plan_set_agg_mode(fsgm_epi_plan* plan, int32_t mode);
/* Adaptive P2 for this plan (fsgm_epi_options.adaptive_p2; 0 at creation).  An adaptive plan resolves to the line kernels
 * whatever its batch ("packed16/nowrap", "packed16/wrap" or "generic"): switching it on after modes 2-6 were forced, and
 * fsgm_epi_plan_set_agg_mode(2..6) on an adaptive plan, return FSGM_ERR_UNSUPPORTED and change nothing.  The aggregate stage
 * then reads the first image of every slot: an aggregation-only plan (fsgm_epi_plan_upload_cost) supplies it through
 * fsgm_epi_plan_upload_images, and a run with a slot whose image was never uploaded returns FSGM_ERR_INVALID before
 * anything is queued.  With 0 every output and every kernel selection is what it was before the switch existed. */
fsgm_status fsgm_epi_plan_set_adaptive_p2(fsgm_epi_plan* plan, int32_t on);
/* The runner-up cost (FSGM_NO_RUNNER_UP above) for this plan, 0 at creation, under the rules of the switch above: with it on
 * the plan resolves to the line kernels whatever its batch, fsgm_epi_plan_set_agg_mode(2..6) returns FSGM_ERR_UNSUPPORTED and
 * changes nothing, and so does switching it on after such a mode was forced.  The first 1 allocates batch * W * H * 4 bytes.  With
 * 0 every output and every kernel selection is what it was; with 1 bestD, minC, conf and bestD2 are those of mode 1. */
fsgm_status fsgm_epi_plan_set_runner_up(fsgm_epi_plan* plan, int32_t on);
/* Exact path arithmetic ("exact" under fsgm_sgm_batch_host_exact below) for this plan, 0 at creation, under the rules of the two
 * switches above: with it on the plan resolves to "packed16/exact" (the dMax classes of the line kernels) or "generic/exact"
 * (every other dMax) whatever its batch, costs and penalties; fsgm_epi_plan_set_agg_mode(2..6) returns FSGM_ERR_UNSUPPORTED and
 * changes nothing, and so does switching it on after such a mode was forced.  It composes with adaptive P2 and not with the
 * runner-up cost: either of the two switches going on while the other is on is FSGM_ERR_UNSUPPORTED.  An exact plan takes P1
 * and P2 in 0..255: fsgm_epi_plan_set_penalties with anything else, and switching it on over such penalties, is
 * FSGM_ERR_INVALID.  Its path volumes hold L_r - C, so fsgm_epi_plan_download_sum rebuilds S from them and the plan's cost
 * volume.  With 0 every output and every kernel selection is what it was. */
fsgm_status fsgm_epi_plan_set_exact(fsgm_epi_plan* plan, int32_t on);
/* The first disparity of a FSGM_SAMPLING_RECTIFIED plan's search range (0 at creation; fsgm_stereo_sgm_host_range above): read
 * by the next cost stage and forward-backward check.  The plan's own outputs stay candidate indices * 256 (fsgm_epi_plan_download,
 * _download_fb with 512 << 8 for invalid).  Any other plan: FSGM_ERR_UNSUPPORTED; |d_min| > FSGM_D_MIN_LIMIT: FSGM_ERR_INVALID;
 * neither touches the device. */
fsgm_status fsgm_epi_plan_set_d_min(fsgm_epi_plan* plan, int32_t d_min);
/* host -> HBM (async on the plan's stream) */
fsgm_status fsgm_epi_plan_upload(fsgm_epi_plan* plan, int32_t frame, const uint8_t* I1,
                                 const uint8_t* I2, const double* pixelPosD0,
                                 const double* normDir, const double* offset);
/* the image pair of slot `frame` alone (any plan; all a rectified plan takes) */
fsgm_status fsgm_epi_plan_upload_images(fsgm_epi_plan* plan, int32_t frame, const uint8_t* I1, const uint8_t* I2);
/* aggregation-only use: put a ready cost volume into slot `frame` (skips FSGM_STAGE_COST) */
fsgm_status fsgm_epi_plan_upload_cost(fsgm_epi_plan* plan, int32_t frame, const uint8_t* C);
/* resident cost volume of frame dst <- frame src with the columns rotated by roll_cols (dst[y][(x + roll) % W] = src[y][x]),
 * device to device on the plan's stream: fills a large batch with distinct volumes without a PCIe transfer each (bench.py) */
fsgm_status fsgm_epi_plan_copy_cost(fsgm_epi_plan* plan, int32_t dst, int32_t src, int32_t roll_cols);
/* offset map only (needed by the vz->disp step when the cost stage is skipped) */
fsgm_status fsgm_epi_plan_upload_offset(fsgm_epi_plan* plan, int32_t frame, const double* offset);
fsgm_status fsgm_epi_plan_run(fsgm_epi_plan* plan, int32_t stages);
fsgm_status fsgm_epi_plan_sync(fsgm_epi_plan* plan);
/* HBM -> host (synchronous) */
fsgm_status fsgm_epi_plan_download(fsgm_epi_plan* plan, int32_t frame, uint32_t* bestD, uint32_t* minC);
fsgm_status fsgm_epi_plan_download_fb(fsgm_epi_plan* plan, int32_t frame, uint8_t* conf, uint32_t* bestD2);
/* minC2 u32 [H][W] of the last FSGM_STAGE_WTA run (every sampling; aggregation-only plans too); FSGM_ERR_INVALID while the
 * plan's runner-up switch is off */
fsgm_status fsgm_epi_plan_download_runner_up(fsgm_epi_plan* plan, int32_t frame, uint32_t* minC2);
fsgm_status fsgm_epi_plan_download_cost(fsgm_epi_plan* plan, int32_t frame, uint8_t* C);
fsgm_status fsgm_epi_plan_download_sum(fsgm_epi_plan* plan, int32_t frame, uint32_t* S);
/* debug tap: the census codes of the two images as FSGM_STAGE_COST left them (common.cpp:3-27; u32 [H][W],
 * the reference's bit order: first tap at bit 25, bit 0 always 0); either pointer may be NULL */
fsgm_status fsgm_epi_plan_download_census(fsgm_epi_plan* plan, int32_t frame, uint32_t* cen1, uint32_t* cen2);
/* Average milliseconds of one fsgm_epi_plan_run(stages) over `iters` back-to-back runs after
 * `warmup` untimed ones, measured with HIP events on the stream the kernels run on. */
fsgm_status fsgm_epi_plan_time(fsgm_epi_plan* plan, int32_t stages, int32_t warmup,
                               int32_t iters, float* ms_avg);
/* the hipStream_t the plan launches on */
void*       fsgm_epi_plan_stream(fsgm_epi_plan* plan);
/* which aggregation kernel the plan selected: "band16/nowrap" (band sweeps, one workgroup per frame: hundreds of frames),
 * "band16chain/nowrap" (band sweeps, the bands of a frame as workgroups of their own), "sweep16/nowrap" (8 paths, block sweep
 * pipeline), "sweep16par/nowrap" (8 paths, parallel sweeps: auto mode for 4..17 frames), "sweep16mid/nowrap" (8 paths, parallel
 * sweeps meeting in the middle), "pairs16/nowrap" (4 paths, pair
 * pipeline), "packed16/nowrap", "packed16/wrap" (per-direction line kernels: dMax = 16, 32, 64, 128, 256 at 16 costs a lane,
 * and 48, 96, 192 / 80, 160 / 112, 224 at 12 / 20 / 28 costs a lane -- these seven take the line kernels at every batch size
 * and under every forced mode, the fused pipelines being built for 16 costs a lane), "generic" (any other dMax, 144, 176, 208
 * and 240 included); on a plan with exact path arithmetic (fsgm_epi_plan_set_exact) "packed16/exact" (the same dMax classes) and
 * "generic/exact" (any other dMax).  New names may be added: dispatch on these with a default branch. */
const char* fsgm_epi_plan_kernel_name(fsgm_epi_plan* plan);
/* The same answer without a plan: what auto mode takes for `batch` frames of width x height x dMax with these penalties, costs
 * up to cmax (24 for volumes built by the cost stage) and a device of `cus` compute units (MI355X: 256).  The switch points
 * were measured at 1242x375x128 and move with the frame's voxels^(-2/3) (smaller frames stay on the line kernels for longer);
 * FSGM_EPI_PAR_MIN / _PAR_MAX / _PAIRS_MIN / _BAND_MIN in the environment override them.  "" for invalid arguments. */
const char* fsgm_epi_auto_pipeline(int32_t width, int32_t height, int32_t dMax, int32_t batch, int32_t paths, int32_t P1, int32_t P2,
                                   int32_t cmax, int32_t cus);
/* the same for a call with options: an adaptive-P2 call takes the line kernels at every batch size */
const char* fsgm_epi_auto_pipeline_opts(int32_t width, int32_t height, int32_t dMax, int32_t batch, int32_t paths, int32_t P1,
                                        int32_t P2, int32_t cmax, int32_t cus, const fsgm_epi_options* opt);
/* Which kernels FSGM_STAGE_COST launches for a plan of width x height x dMax and this sampling (FSGM_SAMPLING_*), written to buf
 * as text: the launchers' own selector evaluated without a device, under the environment as it stands (FSGM_COST_FUSED=0 never
 * fuses, read at every call; FSGM_BOX16=0 never takes the 16-byte box kernel, read once per process).
 *   "costbox"         raw cost and 5x5 box mean in one kernel: dMax = 16, 32, 64, 128, 256 with width < 2^22, height < 2^24
 *   "stereo-costbox"  the same kernel's rectified form (FSGM_SAMPLING_RECTIFIED)
 *   "<raw>+<box>"     the two-kernel form, a raw-cost kernel into a volume in HBM and a box kernel over it:
 *     raw  "px"      one pixel a lane, all d       dMax % 8 == 0 (and width < 2^22, height < 2^24)
 *          "vec4"    four d a thread, one store    dMax % 4 == 0 otherwise
 *          "scalar"  four d a thread, guarded      every other dMax
 *          "stereo"  one voxel a thread            every dMax of a rectified plan
 *     box  "box16"   sliding window, 16 d a lane   dMax % 16 == 0
 *          "box4"    sliding window, 4 d a lane    dMax % 4 == 0 otherwise
 *          "box1"    25 taps a thread              every other dMax
 * FSGM_SAMPLING_VZ and _LINEAR run the same kernels.  Shapes that plan creation refuses are refused here with the same status
 * (FSGM_ERR_INVALID: a size below 1, an unknown sampling; FSGM_ERR_UNSUPPORTED: dMax > 1024, 2^31 voxels or more), a NULL buf
 * or a buflen too small for the name and its terminator with FSGM_ERR_INVALID; buf is "" then (if it can be written at all).
 * 32 bytes hold every name.  New names may be added. */
fsgm_status fsgm_epi_cost_kernels(int32_t width, int32_t height, int32_t dMax, int32_t sampling, char* buf, size_t buflen);
/* device-to-device copy bandwidth probe (GB/s, read+written bytes counted) used by bench.py: the library's own
 * grid-stride copy kernel, 16 B per lane per access -- the access width of the aggregation kernels */
fsgm_status fsgm_measure_copy_bandwidth(int32_t device, size_t bytes, int32_t iters, double* gbps);
/* mode 0: the same; mode 1: hipMemcpyAsync device-to-device (the runtime's blit kernel), for comparison */
fsgm_status fsgm_measure_copy_bandwidth2(int32_t device, size_t bytes, int32_t iters, int32_t mode, double* gbps);

/* sgm(C, P1, P2) -- the call shape of sgm.m:1 / test.m:36 ("perform SGM on cost volume C"), served by the calc_cost_sgm
 * path's aggregation + WTA (calc_cost_sgm.cpp:86-316): C u8 [H][W][dMax] (d fastest) in; bestD u32 [H][W] = disparity
 * index * 256 with the MEX's parabola (no vz conversion), minC u32 [H][W], optionally S u32 [H][W][dMax] out.
 * SEMANTICS ARE THE MEX'S, NOT sgm.m's: path arithmetic is mod 256 where sgm.m saturates (MATLAB uint8), a path's
 * first pixel stores minimum 0 (calc_cost_sgm.cpp:154) where sgm.m takes min(C), and d = 1 is never refined
 * (SURVEY 8(a) note on sgm.m) -- results differ from sgm.m's from the second pixel of every path on.
 * paths: 4 (sgm.m's enableDiagonalPath = false) or 8. */
fsgm_status fsgm_sgm_host(const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1, int32_t P2,
                          int32_t paths, uint32_t* bestD, uint32_t* minC, uint32_t* S, int32_t device);

/* sgm(C, P1, P2) on a batch of caller-supplied volumes, with every aggregation pipeline of the plans within reach (the
 * call above: one frame, a batch-1 plan, the line kernels only).  fsgm_sgm_device, under "Device-pointer entry points"
 * below, is the same call on volumes that are already in HBM.
 * C: n_frames contiguous u8 volumes, each [H][W][dMax] (FSGM_COST_LAYOUT_HWD, d fastest: fsgm_sgm_host's) or [dMax][H][W]
 * (FSGM_COST_LAYOUT_DHW: a contiguous torch (N, D, H, W) tensor, transposed on the device on the way in).
 * bestD, minC u32 [n][H][W] as fsgm_sgm_host's; S (may be NULL) u32 [n][H][W][dMax], d fastest in either layout.
 * cost_bound, 1..255: the caller's declaration that no byte of C is larger.  The pipelines' no-wrap budgets are chosen from
 * it (a volume of small costs reaches the fused pipelines, as census costs <= 24 do), which is why the device form, which
 * may not wait for the device to learn the true maximum, needs it.  The host form scans C as fsgm_sgm_host does and uses
 * min(true maximum, cost_bound); a volume with a byte above a cost_bound below 255 is FSGM_ERR_INVALID and nothing is written.
 * agg_mode: fsgm_epi_plan_set_agg_mode's (0 auto, by n_frames) on the cached plan; plans of different modes are distinct.
 * adaptive_p2 = 1: the reference's edge-aware P2 (fsgm_epi_options), read from guide, the first image, u8 [n][H][W];
 * guide NULL with adaptive_p2 is FSGM_ERR_INVALID, agg_mode 2..6 with it FSGM_ERR_UNSUPPORTED (line kernels only).
 * Refused before a device is touched: n_frames / width / height < 1, dMax outside 1..1024, paths other than 4 or 8, a
 * layout or cost_bound outside the above, subpixel / adaptive_p2 other than 0 or 1, agg_mode outside 0..6, a NULL C, bestD
 * or minC, non-zero reserved words (all FSGM_ERR_INVALID). */
#define FSGM_COST_LAYOUT_HWD 0
#define FSGM_COST_LAYOUT_DHW 1
typedef struct {
    int32_t paths, subpixel, device, agg_mode, layout, cost_bound, adaptive_p2;
    int32_t reserved[5];       /* must be zero */
} fsgm_sgm_params;
fsgm_sgm_params fsgm_sgm_params_default(void);   /* 4, 1, 0, 0 (auto), FSGM_COST_LAYOUT_HWD, 255, 0 */
fsgm_status fsgm_sgm_batch_host(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1,
                                int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                uint32_t* S);
/* fsgm_sgm_batch_host with the runner-up cost (FSGM_NO_RUNNER_UP above, the 1-D rule) minC2 u32 [n][H][W] after minC; minC2
 * must not be NULL (FSGM_ERR_INVALID).  The cached plan has the epipolar plan's runner-up switch on and is never the plan of a
 * call without minC2: such a call runs the line kernels at every batch size (fsgm_sgm_last_kernel shows it), a plain call keeps
 * its plan and pipeline.  agg_mode 2..6 with it is FSGM_ERR_UNSUPPORTED before a device is touched. */
fsgm_status fsgm_sgm_batch_host_ru(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1,
                                   int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                   uint32_t* minC2, uint32_t* S);
/* fsgm_sgm_batch_host with EXACT path arithmetic: the SGM recurrence on integers, for volumes and penalties outside the no-wrap
 * budget cmax + P2 + max(P1, P2) <= 255, where the call above reproduces the MEX's unsigned char overflow (a volume of bytes up
 * to 255 at sgm.m's default P1 = 7, P2 = 100 is far outside it).  Everything is the MEX's (calc_cost_sgm.cpp:86-316) except that
 * a path cost is never narrowed:
 *   path start (:152-180)  L[d] = C[d], stored minimum m = 0 (the quirk is kept);
 *   step                   L[d] = C[d] + min(Lp[d], Lp[d-1] + P1 (d > 0), Lp[d+1] + P1 (d < dMax-1), m_p + P2) - m_p, then
 *                          m = min over d of L[d], the true minimum (the reference's initial 255, :39, is no clamp here);
 *   adaptive P2            P2 / 8 in place of P2 where |I1[cur] - I1[pre]| > 25, per step, as in the call above;
 *   S, WTA, sub-pixel      S = sum over the paths of L in u32; first minimum, the bestIdx > 1 && bestIdx < dMax rule, the
 *                          parabola and bestD = index * 256 (+ sub-pixel) exactly as the call above computes them from S;
 *   passes and paths       pass 1 the point mirror of pass 0, diagonals re-entering at the opposite border, 4 or 8 paths.
 * Then 0 <= L - C <= P2, L <= 255 + P2 and S <= 8 * (255 + P2).  Inside the no-wrap budget the outputs are those of the call
 * above, bit for bit.  P1 and P2 must lie in 0..255 (P1 > P2 is allowed), anything else is FSGM_ERR_INVALID before a device is
 * touched; cost_bound is treated as above (the host form scans C, the device form saturates at it) and selects nothing.
 * The cached plan has the epipolar plan's exact switch on (fsgm_epi_plan_set_exact) and is never the plan of a plain call; it
 * runs the line kernels at every batch size -- fsgm_sgm_last_kernel answers "packed16/exact" or "generic/exact" -- and
 * agg_mode 2..6 with it is FSGM_ERR_UNSUPPORTED before a device is touched.  There is no exact form with minC2. */
fsgm_status fsgm_sgm_batch_host_exact(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                      uint32_t* S);
/* the pipeline (fsgm_epi_plan_kernel_name's names) that the calling thread's last fsgm_sgm_batch_host / fsgm_sgm_device (any
 * of their forms) ran, "" before the first */
const char* fsgm_sgm_last_kernel(void);
/* The static LDS (bytes per workgroup) of the kernel that brings volumes of this layout into a plan, answered without a
 * device: 0 for FSGM_COST_LAYOUT_HWD (a copy), one padded tile for FSGM_COST_LAYOUT_DHW whatever dMax (1..1024) is. */
fsgm_status fsgm_sgm_ingest_lds(int32_t layout, int32_t dMax, uint64_t* bytes);

/* census(img, cen, width, height) of common.cpp:3-27 on its own: u8 [H][W] -> u32 [H][W], 5x5 window, replicate
 * border, `neighbour >= centre`, first tap at bit 25, trailing shift (bit 0 = 0).  Any width/height >= 1. */
fsgm_status fsgm_census_host(const uint8_t* img, int32_t width, int32_t height, uint32_t* cen, int32_t device);

/* ------------------------------------------------------------------------------------------
 * epipolar_sgm_of with the dense maps made on the device  (dense half only)
 *
 * epipolar_geometry.m has a sparse half -- SURF features, an LMedS fundamental matrix, two SVDs and
 * the expansion vote (:30-96) -- the toolbox part of it (:130-149) is NOT built here, the 3x3 algebra from F on is a host helper
 * (fsgm_epipolar_from_F below) -- and a dense half: the
 * per-pixel maps Pd0 / normlizeDirection / Offset / Rflow from F, H, the epipole and the direction
 * flag (:99-115, rotation_motion.m).  The dense half and the tail of epipolar_sgm_of.m (:33-51: gray
 * conversion, calc_cost_sgm, flow = disparity * direction + rotation flow) run on the device, so a
 * call uploads the image pair and 21 numbers instead of 18.6 MB of fp64 maps per 1242x375 frame.
 * Matrices are row-major (F[3*i+j] = F(i+1,j+1)); pixel coordinates as in MATLAB (1-based outputs).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    double F[9];          /* fundamental matrix                                   (epipolar_geometry.m:30) */
    double H[9];          /* rotation-compensating homography K*R/K               (:62) */
    double epipole[2];    /* epipole in image 2, epi(1:2)                          (:43-45) */
    int32_t direction;    /* 0 = expansion, 1 = contraction (directions negated)  (:92-96,:108-110) */
} fsgm_epi_geometry;

/* The in-tree remainder of the sparse half: epipolar_geometry.m:40-96 -- from the fundamental matrix F (however it was estimated:
 * the SURF + LMedS front end, :130-149, is MATLAB toolbox code and not built), the intrinsics K and the inlier matches to the
 * epipole in image 2 (svd(F'), :40-43), H = K*R/K with R the rotation of E = K'FK that is close to the identity (:46-65) and the
 * expansion / contraction vote (:68-96).  3x3 host algebra, no GPU.  pts1 / pts2: n_points x (x, y) in MATLAB's 1-based pixel
 * coordinates; inliers (may be NULL = all) one byte per match.  *ambiguous (may be NULL) = 1 when the diagonal test of :58-62
 * accepts both or neither of the two candidate rotations (the reference's answer then depends on its SVD's signs).  UNPINNED:
 * MATLAB's svd is LAPACK's, this is a Jacobi solver; the quantities used are invariant to an SVD's sign freedoms. */
fsgm_status fsgm_epipolar_from_F(const double* F /* 9, row-major */, const double* K /* 9 */, int32_t n_points, const double* pts1,
                                 const double* pts2, const uint8_t* inliers, fsgm_epi_geometry* out, int32_t* ambiguous);

/* [PrefD0, NormlizeDirection, Offset, Rflow] of epipolar_geometry.m:99-115: f64 [2][H][W] / [H][W] */
fsgm_status fsgm_epipolar_maps_host(const fsgm_epi_geometry* g, int32_t width, int32_t height, double* Pd0,
                                    double* normDirect, double* Offset, double* Rflow, int32_t device);
/* [flow, minC] = epipolar_sgm_of(I0, I1, K, dMax, vMax) from :33 on, the geometry given.  Images u8
 * [channels][H][W] (1 or 3 planes, x fastest); flow f64 [3][H][W] (third plane 1, :51); minC (may be
 * NULL) u32 [H][W].  P1 = 6, P2 = 64 (:19).  prm (may be NULL): paths etc. as for calc_cost_sgm. */
fsgm_status fsgm_epipolar_sgm_of_host(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                      int32_t channels, const fsgm_epi_geometry* g, int32_t dMax, double vMax,
                                      const fsgm_epi_params* prm, double* flow, uint32_t* minC);

/* ------------------------------------------------------------------------------------------
 * calc_pyd_cost_sgm  (calc_pyd_cost_sgm.cpp:439-510, called from pyramidal_sgm.m:50)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const uint8_t* I1;            /* prhs[0]  u8 [H][W] */
    const uint8_t* I2;            /* prhs[1] */
    int32_t width, height;        /* mxGetM / mxGetN of prhs[0] (calc_pyd_cost_sgm.cpp:454-455) */
    const double* preMv;          /* prhs[2]  f64 [2][mvHeight][mvWidth], plane 0 = x; indexed with its own stride */
    int32_t mvWidth, mvHeight;    /* mxGetM(prhs[2]), mxGetN(prhs[2])/2 (:493-494); must be >= width, height */
    int32_t halfSearchWinSizeX;   /* prhs[3] */
    int32_t halfSearchWinSizeY;   /* prhs[4] */
    int32_t aggHalfWinSize;       /* prhs[5] */
    int32_t subPixelRefine;       /* prhs[6] */
    int32_t P1, P2;               /* prhs[7], prhs[8] */
    int32_t enableDiagnalPath;    /* prhs[9]  (bool) */
    int32_t totalPass;            /* prhs[10] */
    int32_t adpativeP2;           /* prhs[11] (bool) */
} fsgm_pyd_in;

typedef struct {
    uint32_t* bestD;              /* plhs[0]  u32 [H][W], 0-based candidate index sx*Sy+sy */
    uint32_t* minC;               /* plhs[1]  u32 [H][W] */
    double*   mvSub;              /* plhs[2]  f64 [2][H][W], plane 0 = x; zeros when subPixelRefine == 0 */
    uint8_t*  C;                  /* optional debug tap: cost volume u8 [H][W][D] (calc_pyd_cost_sgm.cpp:496) */
    uint32_t* S;                  /* optional debug tap: summed path costs u32 [H][W][D] (:125) */
} fsgm_pyd_out;

fsgm_status fsgm_calc_pyd_cost_sgm_host(const fsgm_pyd_in* in, const fsgm_pyd_out* out, int32_t device);
fsgm_status fsgm_calc_pyd_cost_sgm_batch_host(int32_t n_frames, const fsgm_pyd_in* in,
                                              const fsgm_pyd_out* out, int32_t device);
/* The same with the 2-D runner-up cost (FSGM_NO_RUNNER_UP above): minC2s[i] u32 [H][W] of frame i; minC2s or one of its
 * pointers NULL is FSGM_ERR_INVALID.  fsgm_pyd_out stays as it is.  The cached plan is never the one of the call above. */
fsgm_status fsgm_calc_pyd_cost_sgm_batch_host_ru(int32_t n_frames, const fsgm_pyd_in* in, const fsgm_pyd_out* out,
                                                 uint32_t* const* minC2s, int32_t device);

typedef struct fsgm_pyd_plan fsgm_pyd_plan;
fsgm_status fsgm_pyd_plan_create(fsgm_pyd_plan** plan, int32_t width, int32_t height,
                                 int32_t mvWidth, int32_t mvHeight, int32_t halfSearchWinSizeX,
                                 int32_t halfSearchWinSizeY, int32_t aggHalfWinSize, int32_t batch,
                                 int32_t device);
void        fsgm_pyd_plan_destroy(fsgm_pyd_plan* plan);
fsgm_status fsgm_pyd_plan_set_params(fsgm_pyd_plan* plan, int32_t P1, int32_t P2,
                                     int32_t enableDiagnalPath, int32_t totalPass,
                                     int32_t adpativeP2, int32_t subPixelRefine);
fsgm_status fsgm_pyd_plan_upload(fsgm_pyd_plan* plan, int32_t frame, const uint8_t* I1,
                                 const uint8_t* I2, const double* preMv);
fsgm_status fsgm_pyd_plan_upload_cost(fsgm_pyd_plan* plan, int32_t frame, const uint8_t* C);
fsgm_status fsgm_pyd_plan_run(fsgm_pyd_plan* plan, int32_t stages);   /* FSGM_STAGE_* bits */
fsgm_status fsgm_pyd_plan_download(fsgm_pyd_plan* plan, int32_t frame, uint32_t* bestD,
                                   uint32_t* minC, double* mvSub);
fsgm_status fsgm_pyd_plan_download_cost(fsgm_pyd_plan* plan, int32_t frame, uint8_t* C);
fsgm_status fsgm_pyd_plan_download_sum(fsgm_pyd_plan* plan, int32_t frame, uint32_t* S);
fsgm_status fsgm_pyd_plan_time(fsgm_pyd_plan* plan, int32_t stages, int32_t warmup,
                               int32_t iters, float* ms_avg);
/* The 2-D runner-up cost (FSGM_NO_RUNNER_UP above) for this plan, 0 at creation: with the switch on every WTA also writes minC2,
 * u32 [batch][H][W], allocated on first use and all ones until a WTA has run.  The switch changes neither the cost nor the
 * aggregation kernel, nor any other output.  fsgm_pyd_plan_download_runner_up is FSGM_ERR_INVALID while the switch is off. */
fsgm_status fsgm_pyd_plan_set_runner_up(fsgm_pyd_plan* plan, int32_t on);
fsgm_status fsgm_pyd_plan_download_runner_up(fsgm_pyd_plan* plan, int32_t frame, uint32_t* minC2);
/* Exact path arithmetic ("exact" under fsgm_sgm2d_batch_host_exact below) for this plan, 0 at creation: with the switch on
 * FSGM_STAGE_AGGREGATE and FSGM_STAGE_WTA run the two kernels of that section ("generic/exact") at every window and every cost
 * bound, on volumes the plan built from an image pair as on uploaded or ingested ones; the cost stage does not depend on it.
 * P1 and P2 must lie in 0..255: with the switch on fsgm_pyd_plan_set_params refuses anything else, and so does this call for
 * the penalties the plan holds (FSGM_ERR_INVALID, nothing changed).  The path volumes of an exact aggregation hold y = L - C,
 * those of a plain one L: a run of FSGM_STAGE_WTA without FSGM_STAGE_AGGREGATE, fsgm_pyd_plan_download_sum included, is
 * FSGM_ERR_INVALID while the switch differs from what the last aggregation ran with.  The runner-up switch combines with it. */
fsgm_status fsgm_pyd_plan_set_exact(fsgm_pyd_plan* plan, int32_t on);

/* Search windows and launches.  Every entry point on this path accepts a search window with sides 2*half+1 <= 64 (so 63 at
 * the most) and at most 1024 candidates (31x33 = 1023 is the largest count); anything else is FSGM_ERR_UNSUPPORTED before a
 * device is touched.
 * fsgm_pyd_launch_lds: for such a window and an aggregation radius, which kernel the cost stage launches and the dynamic LDS
 * bytes of the launches, computed by the expressions the launchers themselves use; the same refusals as fsgm_pyd_plan_create.
 * No device is touched.
 *   cost_kernel   FSGM_PYD_COST_ROWS (row-packed: windows up to 11x11 with a radius up to 2), _PATCH (one workgroup a pixel,
 *                 while its request stays within 48 KiB) or _CANDIDATE (one thread a candidate, no LDS).  The report is that
 *                 of a one-pixel frame: it holds for every frame below 2^30 pixels, the size up to which the row-packed kernel's
 *                 and the patch kernel's grids are legal (larger frames take _PATCH instead of _ROWS, and _CANDIDATE from
 *                 2^31 - 1 pixels on, which no accepted cost volume reaches)
 *   cost_lds      the request of that launch
 *   patch_lds     what the patch kernel would ask for, whether it runs or not
 *   agg_lds       pyd_agg_kernel's request (any window; the only aggregation kernel for wrapping penalties or windows above 11x11)
 *   rows_agg_lds  the row-packed aggregation kernel's request, 0 for a window it does not take */
#define FSGM_PYD_COST_ROWS 0
#define FSGM_PYD_COST_PATCH 1
#define FSGM_PYD_COST_CANDIDATE 2
fsgm_status fsgm_pyd_launch_lds(int32_t halfSearchWinSizeX, int32_t halfSearchWinSizeY, int32_t aggHalfWinSize,
                                int32_t* cost_kernel, uint64_t* cost_lds, uint64_t* patch_lds, uint64_t* agg_lds,
                                uint64_t* rows_agg_lds);

/* sgm2d(C) -- the 2-D matcher on caller-supplied cost volumes: the hinted-window aggregation, first-minimum WTA and x / y
 * parabolas of calc_pyd_cost_sgm.cpp:114-372 (sgm2d) on a batch of u8 volumes the caller made (a flow network's correlation
 * layer: (N, 81, H, W) for a 9x9 window).  The call shape is sgm2d.m's, whose only input is a ready volume.
 * SEMANTICS ARE THE MEX'S, NOT sgm2d.m's: path arithmetic is mod 256 where sgm2d.m saturates (MATLAB uint8), and a path's
 * first pixel stores minimum 0 (calc_pyd_cost_sgm.cpp:182 etc.) where sgm2d.m takes min(C) -- results differ from sgm2d.m's
 * from the second pixel of every path on.  Float volumes enter through fsgm_sgm2d_float_dptr / fsgm_sgm2d_float_batch_host
 * ("Float cost volumes" below), which quantise them to these bytes on the device.
 * The window is (2*halfX+1) x (2*halfY+1) = Sx x Sy candidates; candidate (sx, sy) stands for the displacement
 * (sx - halfX, sy - halfY) added to the pixel's hint, as in the MEX.  C: n_frames contiguous volumes in one of
 *   FSGM_COST2D_LAYOUT_HWD     [H][W][Sx*Sy], candidate index sx*Sy + sy: the reference's order (calc_pyd_cost_sgm.cpp:392-393,
 *                              x offset slow), what fsgm_pyd_plan_download_cost returns
 *   FSGM_COST2D_LAYOUT_DHW     [Sx*Sy][H][W], channel sx*Sy + sy: a contiguous torch (N, D, H, W) tensor in the reference's order
 *   FSGM_COST2D_LAYOUT_DHW_YX  [Sy*Sx][H][W], channel sy*Sx + sx: the y-slow order correlation layers emit
 * each brought into the plan's own padded volume by one kernel pass on the device (the host form stages the bytes as they
 * came and runs the same kernel).  Whatever the layout, bestD is the reference's candidate index sx*Sy + sy.
 * preMv: the hints, f64 [n][2][mvHeight][mvWidth], plane 0 = x, at least as large as the image; NULL = zero hints (mvWidth
 * and mvHeight are then not read): plain sgm2d.  guide: the first image, u8 [n][H][W], read with adaptive_p2 = 1 only
 * (calc_pyd_cost_sgm.cpp:91-95); NULL with adaptive_p2 is FSGM_ERR_INVALID.
 * bestD, minC u32 [n][H][W]; mvSub f64 [n][2][H][W] (zeros with subpixel = 0); flow (may be NULL) f64 [n][2][H][W] = hint +
 * window offset + mvSub (pyramidal_sgm.m:57-64); S (may be NULL) u32 [n][H][W][Sx*Sy], the summed path costs in reference order.
 * cost_bound, 1..255: the caller's declaration that no byte of C is larger; the aggregation kernels are chosen from it
 * (cost_bound + P2 + max(P1, P2) <= 255 with penalties >= 0: no u8 narrowing changes a value, the row-packed kernels for
 * windows up to 11x11; else the generic, wrapping ones).  The host form scans C and uses min(true maximum, cost_bound); a
 * volume with a byte above a cost_bound below 255 is FSGM_ERR_INVALID and nothing is written.
 * Refused before a device is touched: n_frames / width / height < 1, a negative half size, a layout outside the three,
 * cost_bound outside 1..255, totalPass outside 1..2, diagonal / adaptive_p2 / subpixel other than 0 or 1, non-zero reserved
 * words, a NULL C / bestD / minC / mvSub, a hint map smaller than the image (all FSGM_ERR_INVALID); a side above 64 or more
 * than 1024 candidates, width*height*Sx*Sy >= 2^31 (FSGM_ERR_UNSUPPORTED). */
#define FSGM_COST2D_LAYOUT_HWD 0
#define FSGM_COST2D_LAYOUT_DHW 1
#define FSGM_COST2D_LAYOUT_DHW_YX 2
typedef struct {
    int32_t diagonal, totalPass, adaptive_p2, subpixel, device, layout, cost_bound;
    int32_t reserved[5];       /* must be zero */
} fsgm_sgm2d_params;
fsgm_sgm2d_params fsgm_sgm2d_params_default(void);   /* 1, 2, 0, 1, 0, FSGM_COST2D_LAYOUT_HWD, 255: pyramidal_sgm.m:15-22 */
fsgm_status fsgm_sgm2d_batch_host(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX, int32_t halfY,
                                  int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvWidth,
                                  int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, double* mvSub,
                                  double* flow, uint32_t* S);
/* fsgm_sgm2d_batch_host with the 2-D runner-up cost (FSGM_NO_RUNNER_UP above) minC2 u32 [n][H][W] after minC; minC2 must not be
 * NULL (FSGM_ERR_INVALID before a device is touched).  Its cached plan is never the one of a call without minC2; the
 * aggregation, and with it fsgm_sgm2d_last_kernel, is the one the plain call runs. */
fsgm_status fsgm_sgm2d_batch_host_ru(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX, int32_t halfY,
                                     int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvWidth,
                                     int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                                     double* mvSub, double* flow, uint32_t* S);
/* sgm2d(C) with EXACT path arithmetic: the recurrence of calc_pyd_cost_sgm.cpp:34-89, 114-296 on integers that are never
 * narrowed to unsigned char, where the calls above reproduce the MEX's mod-256 overflow whenever
 * max(C) + P2 + max(P1, P2) > 255 (inside that budget the two agree bit for bit):
 *   path start   L[c] = C[c], stored minimum 0 (the MEX's quirk stays)
 *   step         L[c] = C[c] + min(Lp[ctr], min over the 5x5 around ctr except ctr of Lp + P1, m_p + P2) - m_p, ctr the
 *                hint-shifted centre (int)(s + delta + 0.5) of :46-47, cells outside the window absent, m = min_c L[c]
 * Adaptive P2, the path set, diagonal, totalPass, the mirrored pass, the first-minimum WTA and the parabolas are those of the
 * plain call.  P1 and P2 must lie in 0..255 (FSGM_ERR_INVALID before a device is touched); then L <= 255 + P2 <= 510 and
 * S <= 8 * 510 = 4080.  The argument list is fsgm_sgm2d_batch_host_ru's, with minC2 optional: NULL means not wanted.
 * cost_bound keeps its meaning (a volume above it is refused) but selects no kernel: every exact call runs "generic/exact".
 * The cached plan has the plan's exact switch on (fsgm_pyd_plan_set_exact) and is never the plan of a plain call, nor is the
 * plan of a call with minC2 that of one without. */
fsgm_status fsgm_sgm2d_batch_host_exact(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX,
                                        int32_t halfY, int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv,
                                        int32_t mvWidth, int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                        uint32_t* minC2, double* mvSub, double* flow, uint32_t* S);
/* the aggregation that the calling thread's last fsgm_sgm2d_batch_host / fsgm_sgm2d_device ran, "" before the first: "rows"
 * (row-packed, windows up to 11x11), "rows/wide" (its one-line-a-wave mapping: up to 2 landscape frames), "generic"
 * (pyd_agg_kernel without wrapping), "generic/wrap", or "generic/exact" (the _exact forms) */
const char* fsgm_sgm2d_last_kernel(void);
/* The static LDS (bytes per workgroup) of the kernel that brings volumes of this layout into a plan, answered without a
 * device: 0 for FSGM_COST2D_LAYOUT_HWD (a copy or a repack in registers), one padded tile for the channel-major layouts
 * whatever the window; the same refusals as fsgm_pyd_plan_create's window checks. */
fsgm_status fsgm_sgm2d_ingest_lds(int32_t layout, int32_t halfX, int32_t halfY, uint64_t* bytes);

/* ------------------------------------------------------------------------------------------
 * pyramidal_sgm  (pyramidal_sgm.m:1-77 -- the MATLAB driver around calc_pyd_cost_sgm)
 *
 * The whole level loop on the device: image pyramid (impyramid 'reduce', :28-31), rgb2gray (:44-45),
 * one calc_pyd_cost_sgm per level from coarse to fine (:50), index -> motion vector + previous
 * level's hint + sub-pixel part (:57-64), and 2*imresize(mv, 2, 'nearest') as the next level's hint
 * map (:72).  One upload of the image pair, one download of the flow; the reference's loop crosses
 * the MEX boundary once per level.
 *
 * Images: u8 [channels][height][width], channels = 1 (gray) or 3 (R, G, B planes), x fastest -- what
 * permute(I, [2 1 3]) hands a MEX (pyramidal_sgm.m:44).  Flows: f64 [2][height][width], plane 0 = x.
 * impyramid / rgb2gray / imresize are MATLAB toolbox functions that are not in the reference tree;
 * they follow the published behaviour restated in oracle/fsgm_oracle_pyramid.cpp.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t numPyd;                 /* pyramid levels          (pyramidal_sgm.m:12, default 5; test_psgm.m:33 passes 3) */
    int32_t P1, P2;                 /* penalties               (:15-16: 6, 32) */
    int32_t aggHalfWinSize;         /* cost aggregation window (:17: 2) */
    int32_t verSearchHalfWinSize;   /* search window, y        (:18: 5) */
    int32_t horSearchHalfWinSize;   /* search window, x        (:19: 5) */
    int32_t enableDiagonal;         /* :20: 1 */
    int32_t totalPass;              /* :21: 2 */
    int32_t adaptiveP2;             /* :22: 0 */
    int32_t device;                 /* HIP device ordinal */
} fsgm_pyramid_params;

fsgm_pyramid_params fsgm_pyramid_params_default(void);

/* [mvCurLevel, mvPyd, minC] = pyramidal_sgm(I0, I1, numPyd).  mv: level-1 flow f64 [2][H][W]; minC
 * (may be NULL): level-1 minimum summed path cost u32 [H][W]; mvPyd (may be NULL): numPyd pointers,
 * entry l-1 (if not NULL) receives level l's flow f64 [2][H_l][W_l], H_l = ceil(H_{l-1}/2). */
fsgm_status fsgm_pyramidal_sgm_host(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                    int32_t channels, const fsgm_pyramid_params* prm,
                                    double* mv, uint32_t* minC, double* const* mvPyd);

typedef struct fsgm_pyramid_plan fsgm_pyramid_plan;
fsgm_status fsgm_pyramid_plan_create(fsgm_pyramid_plan** plan, int32_t width, int32_t height,
                                     int32_t channels, const fsgm_pyramid_params* prm);
/* the same with `batch` image pairs resident: every kernel of a level covers all of them (frames are independent; a level
 * still needs the level above).  upload_frame / download_frame address one pair; upload / download are frame 0. */
fsgm_status fsgm_pyramid_plan_create_batch(fsgm_pyramid_plan** plan, int32_t width, int32_t height, int32_t channels,
                                           const fsgm_pyramid_params* params, int32_t batch);
fsgm_status fsgm_pyramid_plan_upload_frame(fsgm_pyramid_plan* plan, int32_t frame, const uint8_t* I0, const uint8_t* I1);
fsgm_status fsgm_pyramid_plan_download_frame(fsgm_pyramid_plan* plan, int32_t frame, int32_t level, double* mv, uint32_t* minC);
void        fsgm_pyramid_plan_destroy(fsgm_pyramid_plan* plan);
/* size of pyramid level `level` (1 = full resolution) */
fsgm_status fsgm_pyramid_plan_level_size(fsgm_pyramid_plan* plan, int32_t level, int32_t* width, int32_t* height);
fsgm_status fsgm_pyramid_plan_upload(fsgm_pyramid_plan* plan, const uint8_t* I0, const uint8_t* I1);
fsgm_status fsgm_pyramid_plan_run(fsgm_pyramid_plan* plan);              /* asynchronous */
/* wait for everything queued on the plan.  Plans are independent (own buffers, own stream): several of them
 * run concurrently when each is started with _run before any is waited for -- the throughput form of the
 * driver loop (pyramidal_sgm.m:37-75 handles one pair at a time) */
fsgm_status fsgm_pyramid_plan_sync(fsgm_pyramid_plan* plan);
/* only the image half of the loop (impyramid, rgb2gray: pyramidal_sgm.m:28-31, 44-45), for callers that run
 * another matcher per level (fsgm_amd.pyramidal_sgm_ng swaps calc_pyd_cost_sgm_ng in); asynchronous */
fsgm_status fsgm_pyramid_plan_run_images(fsgm_pyramid_plan* plan);
/* HBM -> host (synchronous): flow and/or minC of one level; either pointer may be NULL */
fsgm_status fsgm_pyramid_plan_download(fsgm_pyramid_plan* plan, int32_t level, double* mv, uint32_t* minC);
/* debug tap: the gray images calc_pyd_cost_sgm saw at one level (after impyramid and rgb2gray), u8 [H_l][W_l] */
fsgm_status fsgm_pyramid_plan_download_gray(fsgm_pyramid_plan* plan, int32_t level, uint8_t* gray0, uint8_t* gray1);   /* frame 0 */
fsgm_status fsgm_pyramid_plan_download_gray_frame(fsgm_pyramid_plan* plan, int32_t frame, int32_t level, uint8_t* gray0, uint8_t* gray1);
/* average milliseconds of one whole pyramid run (HIP events on the plan's stream) */
fsgm_status fsgm_pyramid_plan_time(fsgm_pyramid_plan* plan, int32_t warmup, int32_t iters, float* ms_avg);
/* The 2-D runner-up cost (FSGM_NO_RUNNER_UP above) of level 1, 0 at creation: with the switch on the last level's WTA also writes
 * minC2 u32 [H][W] per frame; no other level, kernel or output changes.  _download_runner_up (synchronous) is FSGM_ERR_INVALID
 * while the switch is off. */
fsgm_status fsgm_pyramid_plan_set_runner_up(fsgm_pyramid_plan* plan, int32_t on);
fsgm_status fsgm_pyramid_plan_download_runner_up(fsgm_pyramid_plan* plan, int32_t frame, uint32_t* minC2);
/* fsgm_pyramidal_sgm_host with minC2 u32 [H][W] of level 1 after minC; minC2 must not be NULL (FSGM_ERR_INVALID before a device
 * is touched).  Its cached plan is never the one of a call without minC2, nor the reverse. */
fsgm_status fsgm_pyramidal_sgm_host_ru(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                       int32_t channels, const fsgm_pyramid_params* prm,
                                       double* mv, uint32_t* minC, uint32_t* minC2, double* const* mvPyd);
/* The median between levels: pyramidal_sgm.m:66-72 with the commented-out lines :70-71 live and a window size.  mvPyd{l} and
 * every level-1 output stay the unfiltered flow (:66 stores it ahead of :70); for l > 1 the hint map of level l - 1 becomes
 *   2 * imresize(medfilt2(mv(:,:,c), [size size]), 2, 'nearest')      per channel c
 * so the median changes only what the finer levels start from.  size 0 is off (the reference as shipped, and the default), 3 is
 * medfilt2's default window, 5 is vmf.m's; anything else is FSGM_ERR_INVALID.  medfilt2 by the rule of fsgm_vmf_host: zero padding
 * outside the level's W x H, the (size*size+1)/2-th smallest value, NaN above every number (NaN only when more than half the
 * window is), +-Inf as numbers; the sign of a zero that ties at the median is unspecified.  The doubling is exact.  With numPyd 1
 * or size 0 every output equals the plain run bit for bit.  The switch may be set at any numPyd and toggled between runs. */
fsgm_status fsgm_pyramid_plan_set_level_median(fsgm_pyramid_plan* plan, int32_t size);
/* fsgm_pyramidal_sgm_host_ru with the level median after prm.  minC2 may be NULL (not wanted: the plan then runs without the
 * runner-up switch).  level_median is part of the cached plans' key, next to the runner-up switch: a plain or _ru call never gets
 * a plan whose median is on, nor the reverse.  A bad size is refused before a device is touched. */
fsgm_status fsgm_pyramidal_sgm_host_lm(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                       int32_t channels, const fsgm_pyramid_params* prm, int32_t level_median,
                                       double* mv, uint32_t* minC, uint32_t* minC2, double* const* mvPyd);
/* The hint map of the next finer level from n_frames flows, on its own: flow f64 [n][2][H][W] -> next f64 [n][2][2H][2W].  For
 * size 3 or 5 exactly the launch the plans make with the switch on; size 0 is 2 * imresize(flow, 2, 'nearest') (:72).  The
 * device form needs no scratch: the kernel is queued on `stream` itself.  4 * n_frames * width * height must stay below 2^31. */
fsgm_status fsgm_flow_level_hints_host(int32_t n_frames, const double* flow, int32_t width, int32_t height, int32_t size,
                                       double* next, int32_t device);
fsgm_status fsgm_flow_level_hints_device(int32_t n_frames, const double* flow, int32_t width, int32_t height, int32_t size,
                                         double* next, int32_t device, void* stream);

/* ---- the pyramidal level loop with the neighbour-guided matcher ----
 * BASELINE config 4 names calc_pyd_cost_sgm_ng for the pyramidal path.  The reference ships that MEX as a swap-in
 * (same 8 arguments as ng_sgm.m:20) without a driver; this is pyramidal_sgm.m's loop (:24-76) around it: level
 * images by impyramid 'reduce' and rgb2gray (:28-31, :44-45), the coarsest level from a zero hint map (:34), every
 * finer level from 2*imresize(flow, 2, 'nearest') of the level above (:72) -- the MEX returns the flow itself
 * (calc_pyd_cost_sgm_ng.cpp:296-297), so no index-to-vector step.  Everything stays in HBM between levels. */
typedef struct {
    int32_t numPyd;                 /* levels, 1..16 */
    int32_t P1, P2;                 /* ng_sgm.m:7-8: 6, 32 */
    int32_t halfSearchWinSize;      /* ng_sgm.m:20: 1  -> 81 candidates per pixel */
    int32_t aggSize;                /* ng_sgm.m:20: 2 */
    int32_t subPixelRefine;         /* ng_sgm.m:20: 0 */
    int32_t device;
} fsgm_ng_pyramid_params;
fsgm_ng_pyramid_params fsgm_ng_pyramid_params_default(void);
typedef struct fsgm_ng_pyramid_plan fsgm_ng_pyramid_plan;
fsgm_status fsgm_ng_pyramid_plan_create(fsgm_ng_pyramid_plan** plan, int32_t width, int32_t height, int32_t channels,
                                        const fsgm_ng_pyramid_params* prm);
/* the same with `batch` image pairs resident: one run takes all of them through every level together (frames are
 * independent; every kernel of a level covers the whole batch) */
fsgm_status fsgm_ng_pyramid_plan_create_batch(fsgm_ng_pyramid_plan** plan, int32_t width, int32_t height, int32_t channels,
                                              int32_t batch, const fsgm_ng_pyramid_params* prm);
fsgm_status fsgm_ng_pyramid_plan_upload_frame(fsgm_ng_pyramid_plan* plan, int32_t frame, const uint8_t* I0, const uint8_t* I1);
fsgm_status fsgm_ng_pyramid_plan_download_frame(fsgm_ng_pyramid_plan* plan, int32_t frame, int32_t level, double* flow, uint32_t* minC);
void        fsgm_ng_pyramid_plan_destroy(fsgm_ng_pyramid_plan* plan);
fsgm_status fsgm_ng_pyramid_plan_level_size(fsgm_ng_pyramid_plan* plan, int32_t level, int32_t* width, int32_t* height);
fsgm_status fsgm_ng_pyramid_plan_upload(fsgm_ng_pyramid_plan* plan, const uint8_t* I0, const uint8_t* I1);
fsgm_status fsgm_ng_pyramid_plan_run(fsgm_ng_pyramid_plan* plan);        /* asynchronous */
/* flow [2][h][w] and minC [h][w] of `level` (1 = full resolution); either may be NULL */
fsgm_status fsgm_ng_pyramid_plan_download(fsgm_ng_pyramid_plan* plan, int32_t level, double* flow, uint32_t* minC);
fsgm_status fsgm_ng_pyramid_plan_time(fsgm_ng_pyramid_plan* plan, int32_t warmup, int32_t iters, float* ms_avg);
/* one call = the whole loop on a plan cached per shape and parameters: I0, I1 as for fsgm_pyramidal_sgm_host;
 * flow [2][height][width] and minC (may be NULL) of level 1; flowPyd (may be NULL): numPyd pointers, entry l-1
 * receives the flow of level l ([2][h_l][w_l]) or is skipped when NULL */
fsgm_status fsgm_pyramidal_sgm_ng_host(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                       int32_t channels, const fsgm_ng_pyramid_params* prm,
                                       double* flow, uint32_t* minC, double* const* flowPyd);
/* The neighbour-guided runner-up cost (FSGM_NO_RUNNER_UP above) of level 1: switch, download and one-call form as for
 * fsgm_pyramid_plan_set_runner_up / _download_runner_up / fsgm_pyramidal_sgm_host_ru */
fsgm_status fsgm_ng_pyramid_plan_set_runner_up(fsgm_ng_pyramid_plan* plan, int32_t on);
fsgm_status fsgm_ng_pyramid_plan_download_runner_up(fsgm_ng_pyramid_plan* plan, int32_t frame, uint32_t* minC2);
fsgm_status fsgm_pyramidal_sgm_ng_host_ru(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                          int32_t channels, const fsgm_ng_pyramid_params* prm,
                                          double* flow, uint32_t* minC, uint32_t* minC2, double* const* flowPyd);
/* The median between levels, as fsgm_pyramid_plan_set_level_median / fsgm_pyramidal_sgm_host_lm */
fsgm_status fsgm_ng_pyramid_plan_set_level_median(fsgm_ng_pyramid_plan* plan, int32_t size);
fsgm_status fsgm_pyramidal_sgm_ng_host_lm(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                          int32_t channels, const fsgm_ng_pyramid_params* prm, int32_t level_median,
                                          double* flow, uint32_t* minC, uint32_t* minC2, double* const* flowPyd);


/* ------------------------------------------------------------------------------------------
 * Post-processing  (SURVEY 8(f) N3): the MATLAB functions the evaluation script chains after SGM
 * (test.m:45-50) -- speckle_filter.m, calc_disp_from_first.m, forward_backward_check.m,
 * scanline_in_fill.m, vzInd2Disp.m -- one entry point per function, same argument meaning.
 *
 * Maps are f64 [height][width], x fastest; NaN = invalid (MATLAB's NaN).  Pd0 / normDirect are
 * f64 [2][height][width] with plane 0 = x, Pd0 in MATLAB's 1-based pixel coordinates; O is
 * offsetFromPosD0; n = dMax + 1 (test.m:6).  (These are the epipolar maps of calc_cost_sgm above.)
 * ------------------------------------------------------------------------------------------ */
/* speckle_filter.m:1 [imageFiltered, labelImage] = speckle_filter(image, maxDiff, maxSpeckleSize): every
 * 4-connected region (neighbours joined when both valid and |a-b| < maxDiff) of fewer than
 * maxSpeckleSize pixels becomes NaN.  labelImage (may be NULL): i32 [H][W], regions numbered in raster
 * order of their first pixel, 0 where the input is NaN.  Defaults of the original: 2, 100. */
fsgm_status fsgm_speckle_filter_host(const double* image, int32_t width, int32_t height, double maxDiff,
                                     double maxSpeckleSize, double* imageFiltered, int32_t* labelImage,
                                     int32_t device);
/* calc_disp_from_first.m:1 D2 = calc_disp_from_first(D1, Pd0, normDirect, O, vMax, n): -1 where no pixel
 * of D1 lands.  D1 must hold non-negative values or NaN (vz indices are): checked. */
fsgm_status fsgm_calc_disp_from_first_host(const double* D1, int32_t width, int32_t height, const double* Pd0,
                                           const double* normDirect, const double* O, double vMax, double n,
                                           double* D2, int32_t device);
/* forward_backward_check.m:1 D1 = forward_backward_check(D1, D2, Pd0, normDirect, O, vMax, n), threshold 2.0 (:6) */
fsgm_status fsgm_forward_backward_check_host(const double* D1, const double* D2, int32_t width, int32_t height,
                                             const double* Pd0, const double* normDirect, const double* O,
                                             double vMax, double n, double* D1checked, int32_t device);
/* scanline_in_fill.m:2 output = scanline_in_fill(input), one channel (test.m:49 passes a 2-D map) */
fsgm_status fsgm_scanline_in_fill_host(const double* input, int32_t width, int32_t height, double* output,
                                       int32_t device);
/* vzInd2Disp.m:1 D = vzInd2Disp(w, O, vMax, n) */
fsgm_status fsgm_vzind2disp_host(const double* w, const double* O, int32_t width, int32_t height, double vMax,
                                 double n, double* D, int32_t device);
/* vmf.m:1 flowMed = vmf(flow): medfilt2(flow(:,:,c), [5 5]) per channel (zero padding, 13th smallest of 25);
 * flow f64 [channels][H][W], 1..3 channels (test.m:76 passes the 3-plane flow) */
fsgm_status fsgm_vmf_host(const double* flow, int32_t width, int32_t height, int32_t channels, double* flowMed,
                          int32_t device);
/* test.m:45-50 in one call, intermediates resident in HBM:
 *   filterD1 = speckle_filter(D1, 2, 100); filterD2 = calc_disp_from_first(filterD1, ...);
 *   filterD1 = forward_backward_check(filterD1, filterD2, ...); filterD1 = speckle_filter(filterD1, dMax, rows*cols/10);
 *   filterD1 = scanline_in_fill(filterD1); disp = vzInd2Disp(filterD1, O, vMax, n)
 * filterD2 and disp may be NULL. */
fsgm_status fsgm_epi_postprocess_host(const double* D1, int32_t width, int32_t height, const double* Pd0,
                                      const double* normDirect, const double* O, double vMax, double n,
                                      double dMax, double* filterD1, double* filterD2, double* disp,
                                      int32_t device);

/* test.m:45-50 on n_frames maps, one after another: D1, O, filterD1, filterD2, disp f64 [n][H][W], Pd0 / normDirect
 * f64 [n][2][H][W].  Each frame's results are those of fsgm_epi_postprocess_host on that frame alone (one launch per
 * stage for the whole batch; no stage looks across a frame boundary; the second speckle pass's size limit is
 * rows*cols/10 of one frame).  filterD2 / disp may be NULL.  n_frames*width*height must stay below 2^31
 * (FSGM_ERR_UNSUPPORTED, answered before any device is touched). */
fsgm_status fsgm_epi_postprocess_batch_host(int32_t n_frames, const double* D1, int32_t width, int32_t height,
                                            const double* Pd0, const double* normDirect, const double* O, double vMax,
                                            double n, double dMax, double* filterD1, double* filterD2, double* disp,
                                            int32_t device);

typedef struct fsgm_post_plan fsgm_post_plan;
fsgm_status fsgm_post_plan_create(fsgm_post_plan** plan, int32_t width, int32_t height, int32_t device);
void        fsgm_post_plan_destroy(fsgm_post_plan* plan);
/* host -> HBM; any pointer may be NULL to keep what the plan holds */
fsgm_status fsgm_post_plan_upload(fsgm_post_plan* plan, const double* D1, const double* Pd0,
                                  const double* normDirect, const double* O);
fsgm_status fsgm_post_plan_run(fsgm_post_plan* plan, double vMax, double n, double dMax);   /* test.m:45-50, asynchronous */
fsgm_status fsgm_post_plan_download(fsgm_post_plan* plan, double* filterD1, double* filterD2, double* disp);
fsgm_status fsgm_post_plan_time(fsgm_post_plan* plan, double vMax, double n, double dMax, int32_t warmup,
                                int32_t iters, float* ms_avg);

/* ------------------------------------------------------------------------------------------
 * Consistency-checked, filtered flow for the pyramidal matchers.
 *
 * The chain test.m:45-49 applies to the epipolar method's scalar map, on the two-channel flow of fsgm_pyramidal_sgm /
 * fsgm_pyramidal_sgm_ng.  The reference has no such layer for 2-D flow: each stage restates the scalar MATLAB function
 * with the one rule that a vector needs, and those rules are this library's ("Filtered flow for the pyramids").
 * Flows are f64 [2][height][width], plane 0 = u (x); a pixel is valid when neither channel is NaN.
 *
 *  speckle    speckle_filter.m: two 4-connected valid pixels join when |du| < maxDiff and |dv| < maxDiff (strict, :55);
 *             a region of fewer than maxSpeckleSize pixels becomes NaN in both channels.  Invalid pixels are copied.
 *  fb_check   forward_backward_check.m with p2 = round(p + f(p)), p in MATLAB's 1-based pixel coordinates, round half away
 *             from zero (:20): a valid pixel of f becomes NaN (both channels) when p2 is outside the image (:22), b(p2) is
 *             invalid (:27) or |f_u(p) + b_u(p2)| > thr or |f_v(p) + b_v(p2)| > thr (:32).  b is only read.
 *  in_fill    scanline_in_fill.m with lines 16 and 19 restored: the holes are those of channel u (input(v, u) of a 3-D
 *             array is its first plane); interior gaps take min(left, right) per channel, the row ends and then the column
 *             ends copy the nearest vector.  Channel u of the result is fsgm_scanline_in_fill_host of u alone.
 *
 * Every stage takes n_frames contiguous flows.  The host forms copy in and out; the device forms follow the contract of the
 * device-pointer entry points below (caller's stream, pointer checks, captured streams refused; outputs must not overlap
 * inputs).  The scratch lives in a plan cached per width, height, n_frames and device.
 * ------------------------------------------------------------------------------------------ */
fsgm_status fsgm_flow_speckle_filter_host(int32_t n_frames, const double* flow, int32_t width, int32_t height, double maxDiff,
                                          double maxSpeckleSize, double* flowFiltered, int32_t device);
fsgm_status fsgm_flow_speckle_filter_device(int32_t n_frames, const double* flow, int32_t width, int32_t height, double maxDiff,
                                            double maxSpeckleSize, double* flowFiltered, int32_t device, void* stream);
fsgm_status fsgm_flow_fb_check_host(int32_t n_frames, const double* f, const double* b, int32_t width, int32_t height,
                                    double thr, double* fChecked, int32_t device);
/* needs no scratch: the kernel is queued on `stream` itself */
fsgm_status fsgm_flow_fb_check_device(int32_t n_frames, const double* f, const double* b, int32_t width, int32_t height,
                                      double thr, double* fChecked, int32_t device, void* stream);
fsgm_status fsgm_flow_in_fill_host(int32_t n_frames, const double* flow, int32_t width, int32_t height, double* flowFilled,
                                   int32_t device);
fsgm_status fsgm_flow_in_fill_device(int32_t n_frames, const double* flow, int32_t width, int32_t height, double* flowFilled,
                                     int32_t device, void* stream);

#define FSGM_MATCHER_PYD 0   /* fsgm_pyramidal_sgm     (calc_pyd_cost_sgm per level) */
#define FSGM_MATCHER_NG  1   /* fsgm_pyramidal_sgm_ng  (calc_pyd_cost_sgm_ng per level) */
typedef struct {
    int32_t matcher;                /* FSGM_MATCHER_PYD / FSGM_MATCHER_NG */
    fsgm_pyramid_params pyd;        /* the matcher's own parameters (numPyd inside); only the struct of `matcher` is read, */
    fsgm_ng_pyramid_params ng;      /* and its device field is replaced by `device` below */
    double  speckle_max_diff;       /* 2    (test.m:45) */
    double  speckle_max_size;       /* 100  (test.m:45) */
    double  fb_thr;                 /* 2.0  (forward_backward_check.m:6), >= 0 */
    double  island_fraction;        /* 0.1  (test.m:48: rows*cols/10), in [0, 1] */
    int32_t median;                 /* 0; 1 = vmf.m's 5x5 median on the filled flow */
    int32_t device;
} fsgm_flow_pp_params;
/* the defaults of fsgm_pyramid_params_default / fsgm_ng_pyramid_params_default and the values above */
fsgm_flow_pp_params fsgm_flow_pp_params_default(int32_t matcher);

/* n_frames image pairs (I0, I1 u8 [n][channels][H][W]) through one run of a pyramid plan of batch 2n -- frames 0..n-1 match
 * I0 -> I1 (the forward flow f), frames n..2n-1 match I1 -> I0 (the backward flow b) -- and then, without leaving HBM:
 *   f, b = speckle(f, b; speckle_max_diff, speckle_max_size)          one launch sequence over the 2n flows
 *   c    = fb_check(f, b; fb_thr)
 *   c    = speckle(c; +inf, (double)(H*W) * island_fraction)          island removal: any two valid neighbours join
 *   g    = in_fill(c);  g = vmf(g) when median
 * flow_pp      f64 [n][3][H][W]: g's two planes and 1.0 / 0.0 where c is valid / invalid (the layout of
 *              fsgm_epipolar_flow_pp's flow2)
 * flow_checked f64 [n][2][H][W] (may be NULL): c, NaN where rejected
 * flow_fwd, flow_bwd f64 [n][2][H][W] (may be NULL): the raw flows; flow_fwd is what the matcher's own entry point returns
 * minC         u32 [n][H][W] (may be NULL): level-1 minC of the forward run
 * The host form uploads each image once and fills the second half of the plan's input on the device.  The device form
 * follows the device-pointer contract below, except that the images are gathered into the plan's 2n-frame input by two
 * on-device copies per image (u8, H*W*channels bytes a frame) instead of being read where they lie; status (may be NULL)
 * receives 0. */
fsgm_status fsgm_pyramidal_flow_pp_host(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                        int32_t channels, const fsgm_flow_pp_params* prm, double* flow_pp, double* flow_checked,
                                        double* flow_fwd, double* flow_bwd, uint32_t* minC);
fsgm_status fsgm_pyramidal_flow_pp_device(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                          int32_t channels, const fsgm_flow_pp_params* prm, double* flow_pp, double* flow_checked,
                                          double* flow_fwd, double* flow_bwd, uint32_t* minC, void* stream, int32_t* status);
/* The same with the uniqueness test (fsgm_uniqueness_filter_planes_host above, its exact inequality) ahead of the chain.  The
 * plan of 2n pairs runs with its runner-up switch on -- a cached plan of its own -- and both planes of an ambiguous pixel of f
 * and of b are blanked, each flow by its own minC and minC2, before the first speckle filter; the chain treats them like any
 * other rejected pixel.  uniqueness_ratio in [0, 100] (FSGM_ERR_INVALID otherwise); 0 rejects nothing and gives the outputs of
 * the plain forms bit for bit.  flow_fwd and flow_bwd are the raw flows, as above; minC and minC2 u32 [n][H][W] are the forward
 * run's, minC2 (the matcher's own rule: 2-D or neighbour-guided) must not be NULL.  Refusals come before a device is touched. */
fsgm_status fsgm_pyramidal_flow_pp_host_u(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                          int32_t channels, const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio,
                                          double* flow_pp, double* flow_checked, double* flow_fwd, double* flow_bwd, uint32_t* minC,
                                          uint32_t* minC2);
fsgm_status fsgm_pyramidal_flow_pp_device_u(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                            int32_t channels, const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio,
                                            double* flow_pp, double* flow_checked, double* flow_fwd, double* flow_bwd, uint32_t* minC,
                                            uint32_t* minC2, void* stream, int32_t* status);
/* The _u forms with the level median (fsgm_pyramid_plan_set_level_median above) after uniqueness_ratio: the plan of 2n pairs runs
 * both directions with it, and flow_fwd / flow_bwd are the raw level-1 flows of those runs.  minC2 may be NULL exactly when
 * uniqueness_ratio is 0 (the plan then runs without the runner-up switch).  level_median 0 gives the _u forms' outputs. */
fsgm_status fsgm_pyramidal_flow_pp_host_lm(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                           int32_t channels, const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio,
                                           int32_t level_median, double* flow_pp, double* flow_checked, double* flow_fwd,
                                           double* flow_bwd, uint32_t* minC, uint32_t* minC2);
fsgm_status fsgm_pyramidal_flow_pp_device_lm(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                             int32_t channels, const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio,
                                             int32_t level_median, double* flow_pp, double* flow_checked, double* flow_fwd,
                                             double* flow_bwd, uint32_t* minC, uint32_t* minC2, void* stream, int32_t* status);
/* average milliseconds (HIP events on the plan's stream, images uploaded once before) of the batch-2n pyramid run, ms[0],
 * and of the chain behind it, ms[1], for host images as fsgm_pyramidal_flow_pp_host takes them */
fsgm_status fsgm_pyramidal_flow_pp_time(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height,
                                        int32_t channels, const fsgm_flow_pp_params* prm, int32_t warmup, int32_t iters, float* ms);

/* ------------------------------------------------------------------------------------------
 * Rectified stereo: checked, filtered and filled disparity maps.
 *
 * The chain test.m:45-50 applies to the epipolar matcher's vz-index map, behind fsgm_stereo_sgm_*_range, with the rectified
 * geometry substituted into the reference's functions: Pd0 = (x + 1, y + 1) in MATLAB's 1-based coordinates, direction
 * (direction, 0), and disp = d_min + w in place of vzInd2Disp.  w is the candidate-index map bestD / 256: f64, exact, NaN
 * where invalid, >= 0 whatever d_min is (the speckle filter needs non-negative values and calc_disp_from_first.m marks an
 * empty cell with -1); the true disparity of a pixel is d_min + w.
 *
 *  second view  calc_disp_from_first.m:6-47: D2 starts at -1; a pixel with value w offers it to the cells (s0x | s1x, s0y | s1y)
 *               around p2 = (x + 1 + (d_min + w) * direction, y + 1), s0 = floor(p2), s1 = s0 + 1, that lie inside the image;
 *               a cell keeps the largest offer (:25 on non-negative values).  NaN offers nothing.  Row y writes rows y and y + 1.
 *  check        forward_backward_check.m:8-37: a valid pixel becomes NaN when p2x = round(x + 1 + (d_min + w) * direction)
 *               (half away from zero) leaves [1, width], when D2(p2) is -1, or when |w - D2(p2)| > thr.
 *  chain        w1 = speckle_filter(w, speckle_max_diff, speckle_max_size); D2 = second view of w1; c = check(w1, D2);
 *               c = speckle_filter(c, dMax, (double)(height * width) * island_fraction); g = in_fill ? scanline_in_fill(c) : c
 *
 * Maps are f64 [n_frames][height][width]; no stage looks across a frame boundary.  Second view and check run as one kernel
 * with the second-view row in LDS: width <= 8192 (8 * width bytes within 64 KiB), FSGM_ERR_UNSUPPORTED beyond, as is
 * n_frames * width * height >= 2^31; both are answered before a device is touched.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    double  speckle_max_diff;       /* 2    (test.m:45) */
    double  speckle_max_size;       /* 100  (test.m:45) */
    double  fb_threshold;           /* 2.0  (forward_backward_check.m:6), >= 0 */
    double  island_fraction;        /* 0.1  (test.m:48: rows*cols/10), in [0, 1] */
    int32_t in_fill;                /* 1    (test.m:49); 0 = disp_pp is disp_checked */
    int32_t reserved[7];            /* must be zero */
} fsgm_stereo_pp_params;
fsgm_stereo_pp_params fsgm_stereo_pp_params_default(void);

/* the dynamic LDS bytes the row kernel asks for at this width, by the expression its launcher uses; the width refusal of every
 * entry point below.  No device is touched. */
fsgm_status fsgm_stereo_pp_launch_lds(int32_t width, uint64_t* row_lds);

/* fsgm_stereo_sgm_host_range and the chain without leaving HBM.  Arguments as fsgm_stereo_sgm_host_range (prm->fb_check must
 * be 0, FSGM_ERR_INVALID otherwise: the chain has its own check, so the dMax <= 511 of the fixed-point check does not apply)
 * plus pp (NULL = the defaults).  Outputs, [n][H][W] each, every one optional except disp_pp:
 *   disp_pp      f64  d_min + g, NaN where nothing could be filled
 *   disp_checked f64  d_min + c: its NaN pattern is the validity mask of test.m:53
 *   disp, minC   the matcher's raw int32 true disparities * 256 and u32 minC (fsgm_stereo_sgm_host_range's)
 *   disp2        f64  -1 where D2 is empty, d_min + D2 elsewhere
 * The device form follows the device-pointer contract below (caller's stream, pointer checks, captured streams refused, no
 * host wait once the shape is warm; outputs must not overlap); the images are read where they lie; status as
 * fsgm_stereo_sgm_device_range. */
fsgm_status fsgm_stereo_sgm_pp_host(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                    int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt,
                                    int32_t d_min, const fsgm_stereo_pp_params* pp, double* disp_pp, double* disp_checked,
                                    int32_t* disp, uint32_t* minC, double* disp2);
fsgm_status fsgm_stereo_sgm_pp_device(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                      int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt,
                                      int32_t d_min, const fsgm_stereo_pp_params* pp, double* disp_pp, double* disp_checked,
                                      int32_t* disp, uint32_t* minC, double* disp2, void* stream, int32_t* status);
/* The two stages on their own, on maps of arbitrary non-negative doubles or NaN (a negative value is FSGM_ERR_INVALID: the
 * host forms answer on the host, the device forms through status, as fsgm_epi_postprocess_device does).  direction -1 or +1,
 * |d_min| <= FSGM_D_MIN_LIMIT, thr >= 0.  Outputs must not overlap inputs.
 * fsgm_stereo_fb_check: D2 given -- the check of D1 against that map (D2out must be NULL); D2 NULL -- the second-view map is
 * made from D1 itself by the fused row kernel, the form the chain runs, and D2out (may be NULL) receives it. */
fsgm_status fsgm_stereo_disp_from_first_host(int32_t n_frames, const double* D1, int32_t width, int32_t height, int32_t d_min,
                                             int32_t direction, double* D2, int32_t device);
fsgm_status fsgm_stereo_disp_from_first_device(int32_t n_frames, const double* D1, int32_t width, int32_t height, int32_t d_min,
                                               int32_t direction, double* D2, int32_t device, void* stream, int32_t* status);
fsgm_status fsgm_stereo_fb_check_host(int32_t n_frames, const double* D1, const double* D2, int32_t width, int32_t height,
                                      int32_t d_min, int32_t direction, double thr, double* D1checked, double* D2out, int32_t device);
fsgm_status fsgm_stereo_fb_check_device(int32_t n_frames, const double* D1, const double* D2, int32_t width, int32_t height,
                                        int32_t d_min, int32_t direction, double thr, double* D1checked, double* D2out, int32_t device,
                                        void* stream, int32_t* status);
/* average milliseconds (HIP events, warm, host images as fsgm_stereo_sgm_pp_host takes them): ms[0] the matcher, ms[1] the
 * chain, ms[2] the fused row kernel alone, ms[3] the epipolar chain's two generic kernels on explicit rectified maps (a cost
 * comparison: their disparity function differs) */
fsgm_status fsgm_stereo_sgm_pp_time(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                    int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt,
                                    int32_t d_min, const fsgm_stereo_pp_params* pp, int32_t warmup, int32_t iters, float* ms);

/* ------------------------------------------------------------------------------------------
 * calc_pyd_cost_sgm_ng  (calc_pyd_cost_sgm_ng.cpp:448-523; same 8-argument list as the call in
 * ng_sgm.m:20, no caller in the reference tree)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const uint8_t* I1;            /* prhs[0] */
    const uint8_t* I2;            /* prhs[1] */
    int32_t width, height;
    const double* preMv;          /* prhs[2]  f64 [2][mvHeight][mvWidth]; hints are clamped to the map (:392-393) */
    int32_t mvWidth, mvHeight;
    int32_t halfSearchWinSize;    /* prhs[3] */
    int32_t aggSize;              /* prhs[4]  aggregation radius = (int)aggSize/2 (:490) */
    int32_t subPixelRefine;       /* prhs[5] */
    int32_t P1, P2;               /* prhs[6], prhs[7] */
} fsgm_ng_in;

typedef struct {
    uint32_t* minC;               /* plhs[0]  u32 [H][W] */
    double*   flow;               /* plhs[1]  f64 [2][H][W], plane 0 = x */
    uint32_t* S;                  /* optional debug tap: summed path costs u32 [H][W][D], D = 9*(2r+1)^2 */
} fsgm_ng_out;

fsgm_status fsgm_calc_pyd_cost_sgm_ng_host(const fsgm_ng_in* in, const fsgm_ng_out* out, int32_t device);
fsgm_status fsgm_calc_pyd_cost_sgm_ng_batch_host(int32_t n_frames, const fsgm_ng_in* in,
                                                 const fsgm_ng_out* out, int32_t device);
/* The same with the neighbour-guided runner-up cost (FSGM_NO_RUNNER_UP above): minC2 u32 [H][W], minC2s[i] that of frame i.  A
 * NULL minC2, minC2s or one NULL among its entries is FSGM_ERR_INVALID before a device is touched.  fsgm_ng_in and fsgm_ng_out
 * are what they were.  The device-list form below has no such sibling. */
fsgm_status fsgm_calc_pyd_cost_sgm_ng_host_ru(const fsgm_ng_in* in, const fsgm_ng_out* out, uint32_t* minC2, int32_t device);
fsgm_status fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(int32_t n_frames, const fsgm_ng_in* in, const fsgm_ng_out* out,
                                                    uint32_t* const* minC2s, int32_t device);

/* Diagnostics: which aggregation kernel a level of calc_pyd_cost_sgm_ng takes.  All of them give the same results; the choice
 * is one of speed, made per level from the level's shape, the frame count, the FSGM_NG_* environment and -- on the device -- the
 * lengths of the candidate lists without repeats (a 1-in-16 sample of the pixels) and two flags (bit 0: a list longer than 64
 * entries, bit 1: an entry outside the packed 4-byte key's range).
 * fsgm_ng_auto_matcher: what the rule answers for D candidates per pixel, the sum of the sampled list lengths, the sample's pixel
 * count (fsgm_ng_sample_pixels(width * height * frames) for a real level) and the flags: "compact16" / "compact32" / "compact64",
 * "grid", "list", "split2" .. "split4", "lines" or "generic"; "" for a size below 1.  A pure function of its arguments and the
 * environment: no device is touched.
 * fsgm_ng_auto_matcher_lds: the largest dynamic LDS request, in bytes, among the kernels such a level launches (0 for a size
 * below 1).  A level whose request exceeds 64 KiB is refused before anything is queued.  No device is touched.
 * fsgm_ng_last_decision: the name of the kernel that ran and the three statistics of the most recent level that
 * fsgm_calc_pyd_cost_sgm_ng_host / _batch_host ran on `device` (read from that call's scratch memory; FSGM_ERR_INVALID when
 * there is none, or when fsgm_calc_cost_sgm_ng_host has reused the memory since).  A level whose environment and size leave a
 * single kernel reports that kernel and zero statistics. */
const char* fsgm_ng_auto_matcher(int32_t width, int32_t height, int32_t D, int32_t frames, uint64_t list_sum, uint64_t sample_pixels,
                                 uint32_t flags);
uint64_t    fsgm_ng_auto_matcher_lds(int32_t width, int32_t height, int32_t D, int32_t frames);
uint64_t    fsgm_ng_sample_pixels(uint64_t pixels);
fsgm_status fsgm_ng_last_decision(int32_t device, const char** matcher, uint64_t* list_sum, uint64_t* sample_pixels, uint32_t* flags);

/* ------------------------------------------------------------------------------------------
 * calc_cost_sgm_ng  (calc_cost_sgm_ng.cpp:484-526, called from ng_sgm.m:20; prhs[2..5] ignored)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const uint8_t* I1;            /* prhs[0] */
    const uint8_t* I2;            /* prhs[1] */
    int32_t width, height;
    int32_t P1, P2;               /* prhs[6], prhs[7] */
    /* The reference draws 2 x rand() per random hint in raster order (:148-149): 8 per pixel.
     * rand_stream = those draws (fsgm_sgm_ng_rand_draws(width,height) values); NULL makes the
     * library call libc rand() itself, which is what the reference does (process-global state). */
    const int32_t* rand_stream;
} fsgm_otf_in;

typedef struct {
    uint32_t* minC;               /* plhs[0]  u32 [H][W] */
    double*   flow;               /* plhs[1]  f64 [2][H][W] */
} fsgm_otf_out;

int64_t     fsgm_sgm_ng_rand_draws(int32_t width, int32_t height);
fsgm_status fsgm_calc_cost_sgm_ng_host(const fsgm_otf_in* in, const fsgm_otf_out* out, int32_t device);
fsgm_status fsgm_calc_cost_sgm_ng_batch_host(int32_t n_frames, const fsgm_otf_in* in,
                                             const fsgm_otf_out* out, int32_t device);

/* ------------------------------------------------------------------------------------------
 * Device lists: a batch over several GPUs of one node from ONE process  (SURVEY 8(b) "batch variants", 8(e);
 * north_star: the host stays MATLAB -- one process -- and a batch of frames shards across the 8 GPUs of a node).
 *
 * Frame i of the batch runs on devices[i % n_devices]; every list entry gets a host thread of its own that runs its frames
 * through the single-device batch call above (own cached plan, own stream); nothing is exchanged between devices -- frames
 * are independent (calc_cost_sgm.cpp has no state across calls), so there is no collective and no peer copy.  Entries are HIP
 * ordinals taken modulo the number of devices present: {0,1,...,7} is valid on any box, on a one-GPU box all entries share the
 * device and take turns.  Results are identical to single calls whatever the list.  Errors: the first failing entry's status
 * and message, prefixed with the entry.  The MEX gateway calc_cost_sgm takes its list from FSGM_DEVICES=0,1,... when it is
 * handed a batch.
 * ------------------------------------------------------------------------------------------ */
fsgm_status fsgm_calc_cost_sgm_batch_devices_host(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                                  const fsgm_epi_params* prm /* device field ignored */,
                                                  int32_t n_devices, const int32_t* devices);
fsgm_status fsgm_calc_pyd_cost_sgm_batch_devices_host(int32_t n_frames, const fsgm_pyd_in* in, const fsgm_pyd_out* out,
                                                      int32_t n_devices, const int32_t* devices);
fsgm_status fsgm_calc_pyd_cost_sgm_ng_batch_devices_host(int32_t n_frames, const fsgm_ng_in* in, const fsgm_ng_out* out,
                                                         int32_t n_devices, const int32_t* devices);
/* frames whose rand_stream is NULL get their libc rand() draws on the calling thread, in frame order, before they scatter:
 * the draws a sequence of single calls would have made (calc_cost_sgm_ng.cpp:148-149) */
fsgm_status fsgm_calc_cost_sgm_ng_batch_devices_host(int32_t n_frames, const fsgm_otf_in* in, const fsgm_otf_out* out,
                                                     int32_t n_devices, const int32_t* devices);
/* image pairs through the pyramidal drivers: arguments per pair as fsgm_pyramidal_sgm_host / fsgm_pyramidal_sgm_ng_host take them */
typedef struct {
    const uint8_t* I0;
    const uint8_t* I1;
    double*   mv;                 /* level-1 flow f64 [2][H][W] */
    uint32_t* minC;               /* may be NULL */
    double* const* mvPyd;         /* may be NULL: numPyd pointers, per-level flows */
} fsgm_pyramid_pair;
fsgm_status fsgm_pyramidal_sgm_batch_devices_host(int32_t n_pairs, const fsgm_pyramid_pair* pairs, int32_t width, int32_t height,
                                                  int32_t channels, const fsgm_pyramid_params* prm /* device field ignored */,
                                                  int32_t n_devices, const int32_t* devices);
fsgm_status fsgm_pyramidal_sgm_ng_batch_devices_host(int32_t n_pairs, const fsgm_pyramid_pair* pairs, int32_t width, int32_t height,
                                                     int32_t channels, const fsgm_ng_pyramid_params* prm /* device field ignored */,
                                                     int32_t n_devices, const int32_t* devices);
/* "0,1,2" (commas, semicolons or blanks) -> devices[]; returns the number of entries, 0 for an empty / NULL text, -1 for anything
 * that is not a list of non-negative integers */
int32_t fsgm_parse_device_list(const char* text, int32_t* devices, int32_t max_devices);
/* the partition itself, for callers that want to know it: the frames of entry `slot` of a list of n_devices entries
 * (frames may be NULL to get the count only) */
void fsgm_shard_frames(int32_t n_frames, int32_t n_devices, int32_t slot, int32_t* frames, int32_t* count);

/* ------------------------------------------------------------------------------------------
 * Device-pointer entry points: inputs already in HBM, outputs left in HBM, work ordered on the caller's stream
 * (what a torch pipeline on the GPU calls: fsgm_amd/torch_ops.py).
 *
 * All array pointers are device memory of the device named in the params (prm->device / the plan's device).  A batch of
 * n frames is contiguous: frame f of an image at I + f*H*W (RGB: I + f*3*H*W), of a 2-plane map at map + f*2*H*W, etc. --
 * the layouts of the host entry points, one frame after another.  Alignment: every pointer on its element size (u32 4 B,
 * f64 8 B, u8 any).  Pointers are checked before anything is queued (hipPointerGetAttributes / hipMemGetAddressRange):
 * memory of another device, host memory (pinned or not), unregistered pointers, misaligned pointers and arrays that run
 * past the end of their allocation are FSGM_ERR_INVALID.
 *
 * The work is ordered after everything already queued on `stream` (a hipStream_t of that device; NULL = the null stream):
 * the plan's stream waits on an event recorded on `stream`, and after the last kernel of the call -- the plan's internal
 * streams joined back first -- `stream` waits on an event recorded on the plan's stream.  Everything queued on `stream`
 * after the call returns runs after it.  Calls from several streams that share one cached plan serialise on that plan's
 * stream; memory the caller frees after the call is only reused by work ordered after the join.
 * No host<->device copy and no wait for the device once a plan for this shape and these parameters exists (the first call
 * may create the plan and upload its tables).  The caller's arrays are read and written where they lie; the plans' own
 * buffers of the host entry points are not touched for them.
 * status (device memory, may be NULL): one int32, written on `stream` at the end -- 0, or FSGM_ERR_HIP when a bounded
 * hand-off poll of the aggregation gave up (what fsgm_epi_plan_sync reports on the host paths).
 * A stream that is being captured into a graph is refused with FSGM_ERR_UNSUPPORTED before anything is queued.
 * The debug taps (out->C / out->S, per-level pyramid flows) are not offered: a non-NULL C or S is FSGM_ERR_UNSUPPORTED
 * (fsgm_sgm_device and fsgm_sgm2d_device alone offer S).
 * Results are bit for bit those of the host entry points for the same inputs.
 * ------------------------------------------------------------------------------------------ */
/* All `batch` frames of a plan (n_frames must equal the plan's batch), cost stage + aggregation + WTA in the plan's
 * aggregation mode (fsgm_epi_plan_set_agg_mode); in->width / height / dMax must match the plan, in->P1 / P2 / vMax
 * are set on it.  bestD, minC, and with fb_check conf / bestD2 (each may be NULL there) as for the host entry points. */
fsgm_status fsgm_epi_plan_run_device(fsgm_epi_plan* plan, int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                     void* stream, int32_t* status);
/* calc_cost_sgm on n_frames contiguous frames (one cached plan of batch n_frames, as fsgm_calc_cost_sgm_batch_host) */
fsgm_status fsgm_calc_cost_sgm_device(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                      const fsgm_epi_params* prm, void* stream, int32_t* status);
/* fsgm_calc_cost_sgm_linear_batch_host on n_frames contiguous frames: in->offset is not read (may be NULL) */
fsgm_status fsgm_calc_cost_sgm_linear_device(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                             const fsgm_epi_params* prm, void* stream, int32_t* status);
/* the two above with options (fsgm_epi_options; the cached plans of adaptive and non-adaptive calls are distinct) */
fsgm_status fsgm_calc_cost_sgm_device_opts(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                           const fsgm_epi_params* prm, const fsgm_epi_options* opt, void* stream, int32_t* status);
fsgm_status fsgm_calc_cost_sgm_linear_device_opts(int32_t n_frames, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                                  const fsgm_epi_params* prm, const fsgm_epi_options* opt, void* stream,
                                                  int32_t* status);
/* fsgm_stereo_sgm_host on device pointers (one cached rectified plan of batch n_frames) */
fsgm_status fsgm_stereo_sgm_device(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                   int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp,
                                   uint32_t* minC, uint8_t* conf, uint32_t* disp2, void* stream, int32_t* status);
fsgm_status fsgm_stereo_sgm_device_opts(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                        int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                        const fsgm_epi_options* opt, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2,
                                        void* stream, int32_t* status);
/* fsgm_stereo_sgm_host_range on device pointers: disp / disp2 int32 true disparities * 256 (disp2 INT32_MIN where invalid); the
 * rules of the entry points above (the caller's stream, no graph capture, no host memory, no C / S taps) */
fsgm_status fsgm_stereo_sgm_device_range(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                         int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                         const fsgm_epi_options* opt, int32_t d_min, int32_t* disp, uint32_t* minC, uint8_t* conf,
                                         int32_t* disp2, void* stream, int32_t* status);
/* fsgm_stereo_sgm_host_ru on device pointers: minC2 (required, checked like minC) is written where it lies by the WTA kernel */
fsgm_status fsgm_stereo_sgm_device_ru(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                      int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm,
                                      const fsgm_epi_options* opt, int32_t d_min, int32_t* disp, uint32_t* minC, uint32_t* minC2,
                                      uint8_t* conf, int32_t* disp2, void* stream, int32_t* status);
/* fsgm_sgm_batch_host on device pointers (one cached plan of batch n_frames per shape, paths, agg_mode and adaptive_p2): C in
 * either layout is brought into the plan's own volume by one kernel pass that stores min(byte, prm->cost_bound), then the
 * aggregation and WTA selected for cost_bound run on it -- saturating keeps every kernel inside the no-wrap budget it was
 * selected for.  status: 0, FSGM_ERR_HIP when an aggregation hand-off gave up, or FSGM_ERR_INVALID when some byte of C was
 * above cost_bound: the outputs are then those of the saturated volume.  guide (adaptive_p2) is copied device to device.
 * Unlike every other entry point of this section this one offers S (may be NULL; device memory, u32 [n][H][W][dMax]): it is
 * rebuilt frame by frame after the run, as fsgm_epi_plan_download_sum does, and copied device to device.  Everything else
 * follows the contract above. */
fsgm_status fsgm_sgm_device(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1, int32_t P2,
                            const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S,
                            void* stream, int32_t* status);
/* fsgm_sgm_batch_host_ru on device pointers: minC2 (required, device memory, checked like minC) is written where it lies by the
 * WTA itself, on the caller's stream; everything else as fsgm_sgm_device. */
fsgm_status fsgm_sgm_device_ru(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1, int32_t P2,
                               const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                               uint32_t* S, void* stream, int32_t* status);
/* fsgm_sgm_batch_host_exact on device pointers: exact path arithmetic (see there), everything else -- ingest saturating at
 * cost_bound, the status word, S -- as fsgm_sgm_device, with one exception to this section's contract: a stream that is being
 * captured into a graph is accepted.  Once the same call (shape, n_frames, paths, switches, with or without S and guide) has run
 * outside a capture, the cached plan and its buffers exist and a call allocates nothing and waits for nothing: the capture records
 * the plan's stream as a branch between two events.  A captured call whose plan or buffers do not exist yet is
 * FSGM_ERR_UNSUPPORTED before anything is queued or allocated.
 * Lifetime: the graph names the caller's arrays AND the cached plan's buffers, stream and events.  The plan is pinned from the
 * captured call on -- never evicted by later calls of other shapes, held beside the usual number of cached plans -- and is
 * destroyed by fsgm_shutdown alone: the graph may be replayed while the caller's arrays live and until fsgm_shutdown.
 * Ordering: a replay is ordered by the stream the graph is launched on, not by the plan's stream.  A later or earlier
 * fsgm_sgm_device_exact call of the same shape on that same stream is ordered against the replay by its event join; calls of the
 * same shape and switches from another stream or thread, and fsgm_sgm_batch_host_exact of that shape, share the plan's buffers
 * with the graph and are NOT ordered against a replay: the caller must keep them apart (an event or a synchronise). */
fsgm_status fsgm_sgm_device_exact(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1,
                                  int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                  uint32_t* S, void* stream, int32_t* status);
/* The first step of fsgm_sgm_device on its own, into a caller's plan: n_frames (= the plan's batch) volumes in `layout` from
 * device memory into the plan's cost volumes (what fsgm_epi_plan_upload_cost fills from the host), saturated at cost_bound,
 * which becomes the bound the plan selects its kernels by.  status: 0 or FSGM_ERR_INVALID (a byte above cost_bound). */
fsgm_status fsgm_epi_plan_ingest_cost_device(fsgm_epi_plan* plan, int32_t n_frames, const uint8_t* C, int32_t layout,
                                             int32_t cost_bound, void* stream, int32_t* status);
/* fsgm_sgm2d_batch_host on device pointers (one cached aggregation-only plan of batch n_frames per shape, window, hint-map
 * size and adaptive_p2, shared with the host form).  C in any of the three layouts is brought into the
 * plan's padded volume by one kernel pass that stores min(byte, prm->cost_bound) and writes the padding as 0; then the
 * aggregation selected for cost_bound and the WTA run on it.  preMv (may be NULL: zero hints), guide (adaptive_p2), bestD,
 * minC, mvSub, flow (may be NULL) and S (may be NULL) are read and written where they lie.  status: 0, or FSGM_ERR_INVALID
 * when some byte of C was above cost_bound: the outputs are then those of the saturated volume.  Everything else follows the
 * contract above. */
fsgm_status fsgm_sgm2d_device(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX, int32_t halfY,
                              int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvWidth,
                              int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, double* mvSub, double* flow,
                              uint32_t* S, void* stream, int32_t* status);
/* fsgm_sgm2d_batch_host_ru on device pointers: minC2 (required, device memory, checked like minC) is written where it lies by
 * the WTA itself, on the caller's stream; everything else as fsgm_sgm2d_device. */
fsgm_status fsgm_sgm2d_device_ru(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX, int32_t halfY,
                                 int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvWidth,
                                 int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                                 double* mvSub, double* flow, uint32_t* S, void* stream, int32_t* status);
/* fsgm_sgm2d_batch_host_exact on device pointers: exact path arithmetic (see there).  minC2 may be NULL (not wanted); when
 * given it is device memory, checked like minC and written by the WTA itself.  The ingest saturates at cost_bound and raises
 * the status word as in fsgm_sgm2d_device; the outputs are then those of the saturated volume under the exact recurrence.
 * Everything else follows the contract above: a stream that is being captured is refused. */
fsgm_status fsgm_sgm2d_device_exact(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t halfX, int32_t halfY,
                                    int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvWidth,
                                    int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                                    double* mvSub, double* flow, uint32_t* S, void* stream, int32_t* status);
/* The first step of fsgm_sgm2d_device on its own, into a caller's plan: n_frames (= the plan's batch) volumes in a
 * FSGM_COST2D_LAYOUT_* from device memory into the plan's cost volumes (what fsgm_pyd_plan_upload_cost fills from the host),
 * saturated at cost_bound, which becomes the bound the plan selects its aggregation by.  status: 0 or FSGM_ERR_INVALID. */
fsgm_status fsgm_pyd_plan_ingest_cost_device(fsgm_pyd_plan* plan, int32_t n_frames, const uint8_t* C, int32_t layout,
                                             int32_t cost_bound, void* stream, int32_t* status);
/* epipolar_sgm_of on n_frames image pairs, one plan of batch n_frames: g (HOST memory) holds n_frames geometries, each
 * passed to the maps kernel by value.  I0 / I1 u8 [n][channels][H][W]; flow f64 [n][3][H][W]; minC (may be NULL) u32 [n][H][W]. */
fsgm_status fsgm_epipolar_sgm_of_device(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                        int32_t height, int32_t channels, const fsgm_epi_geometry* g,
                                        int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                        double* flow, uint32_t* minC, void* stream, int32_t* status);
/* fsgm_epi_postprocess_batch_host on device pointers, ordered on `stream` (a cached post-processing plan per width,
 * height, n_frames and device holds the scratch; outputs must not overlap the inputs).  filterD2 / disp may be NULL.
 * status (may be NULL): 0, or FSGM_ERR_INVALID when some D1 value is negative -- the host entry points refuse such maps
 * on the host; here the chain still runs (every write stays in bounds) and its results are meaningless. */
fsgm_status fsgm_epi_postprocess_device(int32_t n_frames, const double* D1, int32_t width, int32_t height,
                                        const double* Pd0, const double* normDirect, const double* O, double vMax,
                                        double n, double dMax, double* filterD1, double* filterD2, double* disp,
                                        int32_t device, void* stream, int32_t* status);
/* vmf.m on n_frames flows f64 [n][channels][H][W] (1..3 channels): flowMed of the same layout.  Needs no scratch: the
 * kernel is queued on `stream` itself. */
fsgm_status fsgm_vmf_device(int32_t n_frames, const double* flow, int32_t width, int32_t height, int32_t channels,
                            double* flowMed, int32_t device, void* stream);
/* test.m's frame body (:32-54) with the sparse geometry given, on n_frames image pairs (one epi plan of batch n_frames
 * with vz_to_disp = 0, cached apart from epipolar_sgm_of's): gray conversion of RGB input, the epipolar maps,
 * calc_cost_sgm in vz-index mode with P1 = 6, P2 = 64 (:36), D1 = bestD/256, flow (:38-42), the chain of :45-49 with
 * n = dMax + 1 (:6), flow2 (:50-54).  Nothing leaves HBM between the matcher and flow2.
 * D1 is the MEX's vz index (calc_cost_sgm's WTA, 1/256 steps); test.m's own D1 comes from calc_cost.m + sgm.m, which differ
 * from the MEX as described for fsgm_sgm_host.
 * I0 / I1 u8 [n][channels][H][W] (1 or 3 planes); g holds n geometries (HOST memory); flow, flow2 f64 [n][3][H][W]
 * (third plane: 1 where D1 / filterD1 is valid); D1 (may be NULL) f64 [n][H][W]; minC (may be NULL) u32 [n][H][W].
 * prm (may be NULL): paths, subpixel and device honoured, vz_to_disp ignored, fb_check must be 0.
 * The device form follows the contract above; its status word means what it means for fsgm_epipolar_sgm_of_device. */
fsgm_status fsgm_epipolar_flow_pp_host(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                       int32_t height, int32_t channels, const fsgm_epi_geometry* g, int32_t dMax,
                                       double vMax, const fsgm_epi_params* prm, double* flow, double* flow2, double* D1,
                                       uint32_t* minC);
fsgm_status fsgm_epipolar_flow_pp_device(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                         int32_t height, int32_t channels, const fsgm_epi_geometry* g, int32_t dMax,
                                         double vMax, const fsgm_epi_params* prm, double* flow, double* flow2, double* D1,
                                         uint32_t* minC, void* stream, int32_t* status);
/* the pyramids on n_frames image pairs (one plan of batch n_frames): the level-1 flow f64 [n][2][H][W] and minC (may be
 * NULL) u32 [n][H][W].  The level-1 images are read in place by the first reduce / gray / census kernels. */
fsgm_status fsgm_pyramidal_sgm_device(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                      int32_t height, int32_t channels, const fsgm_pyramid_params* prm,
                                      double* mv, uint32_t* minC, void* stream, int32_t* status);
fsgm_status fsgm_pyramidal_sgm_ng_device(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                         int32_t height, int32_t channels, const fsgm_ng_pyramid_params* prm,
                                         double* flow, uint32_t* minC, void* stream, int32_t* status);
/* the same with level 1's runner-up cost minC2 u32 [n][H][W] (required, device memory, checked like minC), written where it lies
 * by the last level's WTA; a cached plan of its own */
fsgm_status fsgm_pyramidal_sgm_device_ru(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                         int32_t height, int32_t channels, const fsgm_pyramid_params* prm,
                                         double* mv, uint32_t* minC, uint32_t* minC2, void* stream, int32_t* status);
fsgm_status fsgm_pyramidal_sgm_ng_device_ru(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                            int32_t height, int32_t channels, const fsgm_ng_pyramid_params* prm,
                                            double* flow, uint32_t* minC, uint32_t* minC2, void* stream, int32_t* status);
/* the same with the level median after prm (fsgm_pyramidal_sgm_host_lm); minC2 may be NULL: not wanted */
fsgm_status fsgm_pyramidal_sgm_device_lm(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                         int32_t height, int32_t channels, const fsgm_pyramid_params* prm, int32_t level_median,
                                         double* mv, uint32_t* minC, uint32_t* minC2, void* stream, int32_t* status);
fsgm_status fsgm_pyramidal_sgm_ng_device_lm(int32_t n_frames, const uint8_t* I0, const uint8_t* I1, int32_t width,
                                            int32_t height, int32_t channels, const fsgm_ng_pyramid_params* prm, int32_t level_median,
                                            double* flow, uint32_t* minC, uint32_t* minC2, void* stream, int32_t* status);

/* ------------------------------------------------------------------------------------------
 * Float cost volumes for sgm(C) and sgm2d(C): a learned matching cost arrives as float32, float16 or bfloat16.  The entries
 * below take such a volume, quantise it to the u8 volume of the entries above in the one kernel pass that brings it into the
 * plan (5 bytes of traffic per fp32 voxel: 4 read, 1 written), and run the existing u8 path on it.
 *
 * THE RULE.  A cost format is {dtype, scale, offset}: dtype one of FSGM_COST_F32 / _F16 / _BF16, scale and offset fp32, both
 * finite, scale != 0 (a negative scale turns a similarity into a cost).  For a voxel c and the call's cost_bound B in 1..255:
 *   1. x = c widened to fp32 (exact for all three types);
 *   2. t = x * scale, one IEEE fp32 multiply, round to nearest even;
 *   3. u = t + offset, one IEEE fp32 add -- the two are never contracted into a fused multiply-add;
 *   4. r = rint(u), ties to even (np.rint);
 *   5. q = 0 if r < 0; q = B if r > B or u is NaN; otherwise q = (uint8) r.  -0.0 gives 0 and is not out of range.
 * A voxel with r < 0, r > B or NaN raises the ingest flag, as a byte above the bound does in the u8 entries: the device forms
 * set the status word to FSGM_ERR_INVALID and their outputs are those of the clamped volume; the host forms return
 * FSGM_ERR_INVALID and write no output.  fp32 subnormal inputs and products are outside the contract (a device may flush them);
 * fp16 and bf16 subnormals are normal fp32 values once widened and are inside it.
 * UNPINNED BY CONSTRUCTION: the reference has no float volumes.  The rule is restated in numpy (tests/cost_quant_restatement.py),
 * and since everything behind the ingest is the u8 path, the yardstick is equality: the outputs of a float call are, bit for
 * bit, those of the u8 call on the restatement's bytes with the same cost_bound.
 *
 * The kernels are chosen from the declared cost_bound exactly as in the u8 device forms -- in the host float forms too, which
 * do not scan for the true maximum: a result never depends on the pipeline that computed it.
 * Refused before a device is touched: everything the u8 forms refuse, and (FSGM_ERR_INVALID) a NULL fmt, an unknown dtype, a
 * non-finite or zero scale, a non-finite offset, non-zero reserved words.  C is aligned on its element size (4 or 2 bytes) and
 * no further: it may be a slice of a larger tensor.
 * ------------------------------------------------------------------------------------------ */
#define FSGM_COST_F32 0
#define FSGM_COST_F16 1
#define FSGM_COST_BF16 2
typedef struct {
    int32_t dtype;             /* FSGM_COST_* */
    float scale, offset;
    int32_t reserved[5];       /* must be zero */
} fsgm_cost_format;
fsgm_cost_format fsgm_cost_format_default(void);   /* FSGM_COST_F32, 1, 0 */
/* fsgm_epi_plan_ingest_cost_device / fsgm_pyd_plan_ingest_cost_device for a float volume: n_frames (= the plan's batch) volumes
 * of fmt->dtype in `layout` from device memory, quantised into the plan's cost volumes; cost_bound becomes the bound the plan
 * selects its kernels by.  status: 0 or FSGM_ERR_INVALID (a flagged voxel).  The contract of the device-pointer entry points. */
fsgm_status fsgm_epi_plan_ingest_float_dptr(fsgm_epi_plan* plan, int32_t n_frames, const void* C, const fsgm_cost_format* fmt,
                                            int32_t layout, int32_t cost_bound, void* stream, int32_t* status);
fsgm_status fsgm_pyd_plan_ingest_float_dptr(fsgm_pyd_plan* plan, int32_t n_frames, const void* C, const fsgm_cost_format* fmt,
                                            int32_t layout, int32_t cost_bound, void* stream, int32_t* status);
/* sgm(C) on float volumes in device memory: what fsgm_sgm_device, _ru and _exact cover together.  minC2 may be NULL (not
 * wanted); exact = 1 selects exact path arithmetic (fsgm_sgm_batch_host_exact).  The cached plans and the internal bodies are
 * those of the u8 forms: only the ingest launch differs.  Refusals are theirs: exact with minC2, and agg_mode 2..6 with exact,
 * minC2 or adaptive_p2, are FSGM_ERR_UNSUPPORTED; a stream that is being captured is refused, with exact too. */
fsgm_status fsgm_sgm_float_dptr(int32_t n_frames, const void* C, const fsgm_cost_format* fmt, int32_t width, int32_t height, int32_t dMax,
                                int32_t P1, int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                uint32_t* minC2, uint32_t* S, int32_t exact, void* stream, int32_t* status);
/* sgm2d(C) on float volumes in device memory: what fsgm_sgm2d_device, _ru and _exact cover together (minC2 may be NULL with or
 * without exact). */
fsgm_status fsgm_sgm2d_float_dptr(int32_t n_frames, const void* C, const fsgm_cost_format* fmt, int32_t width, int32_t height,
                                  int32_t halfX, int32_t halfY, int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv,
                                  int32_t mvWidth, int32_t mvHeight, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                  uint32_t* minC2, double* mvSub, double* flow, uint32_t* S, int32_t exact, void* stream,
                                  int32_t* status);
/* The same on host memory: the caller's floats are staged frame by frame and quantised by the same kernels; the ingest flag is
 * read before any output is written (a flagged volume: FSGM_ERR_INVALID, the outputs untouched). */
fsgm_status fsgm_sgm_float_batch_host(int32_t n_frames, const void* C, const fsgm_cost_format* fmt, int32_t width, int32_t height,
                                      int32_t dMax, int32_t P1, int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide,
                                      uint32_t* bestD, uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact);
fsgm_status fsgm_sgm2d_float_batch_host(int32_t n_frames, const void* C, const fsgm_cost_format* fmt, int32_t width, int32_t height,
                                        int32_t halfX, int32_t halfY, int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm,
                                        const double* preMv, int32_t mvWidth, int32_t mvHeight, const uint8_t* guide, uint32_t* bestD,
                                        uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow, uint32_t* S, int32_t exact);

/* ------------------------------------------------------------------------------------------
 * Second view: the second view's disparity taken from the SAME aggregated volume, and the left-right check against it
 * (Hirschmueller's D_m, OpenCV's disp12MaxDiff).  No second aggregation runs: a kernel of its own reads the path volumes the
 * line kernels' WTA has just read.
 *
 * THE RULE.  S[y][x][i], i in [0, dMax), is the u32 sum of the path volumes exactly as fsgm_epi_plan_download_sum defines it
 * for the plan that ran (wrapped or not; ndirs * C + the sum of the y_r for an exact plan).  s = direction is -1 or +1,
 * delta(i) = d_min + i, and candidate i of first-view pixel (x, y) is second-view pixel (x + s * delta(i), y) -- the
 * convention of fsgm_stereo_sgm_*.  For second-view pixel (x2, y):
 *   candidates  I(x2) = { i : 0 <= x2 - s * delta(i) < width }.  Only a candidate whose unclamped target is x2 counts: the
 *               clamped border samples of the stereo cost stage do not;
 *   winner      i* = the first minimum, in ascending i over I(x2), of S[y][x2 - s * delta(i)][i]; minC_v2 is that value;
 *   empty I(x2) disp2 = the invalid marker, minC_v2 = 0xFFFFFFFF;
 *   sub-pixel   when the call's subpixel is 1 and both i* - 1 and i* + 1 are in I(x2): c_1 and c1 are S at those two diagonal
 *               neighbours, c = minC_v2, and with f64 operations in this order
 *                 sub = i* + ((c1 - c_1) / (c - c_1)) / 2   if c1 < c_1,   sub = i* + ((c1 - c_1) / (c - c1)) / 2   otherwise
 *               (the first view's parabola); disp2 = (u32) trunc(sub * 256).  Otherwise disp2 = i* * 256.  Since i* is a FIRST
 *               minimum, c_1 > c and c1 >= c: the divisor is c - c_1 < 0 in the first branch and c - c1 <= c - c_1 < 0 in the
 *               second -- never zero.  The first view's `best > 1` quirk and its read of the next pixel's d = 0 are not mirrored.
 * Formats: the sgm(C) forms and the plan return disp2 u32 in index units like bestD, marker FSGM_NO_VIEW2; the stereo forms
 * return int32 true disparities * 256 (256 * d_min + the above) like the _range forms, marker INT32_MIN.
 * THE CHECK (integers only).  d1 = the first view's true disparity * 256 (sgm(C): bestD + 256 * d_min; in a call with subpixel = 0
 * the first view returns the whole index, which the one-shot forms scale by 256 first), d2 likewise from disp2:
 *   x2 = x + s * ((d1 + 128) >> 8)   (arithmetic shift, no clamp)
 *   conf[y][x] = 1 iff 0 <= x2 < width, disp2[y][x2] is valid and |d1 - d2| <= max_diff (int64; max_diff >= 0 in 1/256 units,
 *   default 256 = one disparity), else 0.
 * UNPINNED BY CONSTRUCTION: the reference has nothing like it (its fb_check splats the first view's own disparities).  The rule
 * is restated in numpy (tests/view2_restatement.py); the yardstick is equality with the restatement on the S the same call
 * returns.
 *
 * Plans.  fsgm_epi_plan_set_view2(plan, 1, direction): every FSGM_STAGE_WTA run also writes the second view, read by
 * fsgm_epi_plan_download_view2 (frame's disp2 and minC_v2, u32 [H][W], either may be NULL; index units; FSGM_ERR_INVALID while
 * the switch is off).  Such a plan aggregates with the line kernels at every batch size (the fused pipelines keep no volumes);
 * fsgm_epi_plan_set_agg_mode(2..6) on it, and the switch on a plan forced to such a mode, are FSGM_ERR_UNSUPPORTED.  It is
 * FSGM_ERR_UNSUPPORTED on a linear plan (per-pixel direction maps) and on a vz plan with vz_to_disp (the vz sampling): candidates
 * there share no line.  A rectified plan takes its own direction only (FSGM_ERR_INVALID otherwise) and its d_min
 * (fsgm_epi_plan_set_d_min); a vz plan without vz_to_disp serves uploaded cost volumes (d_min 0), and running its own cost stage
 * with the switch on is FSGM_ERR_INVALID.  It composes with adaptive_p2, the runner-up switch and the exact switch.
 * ------------------------------------------------------------------------------------------ */
#define FSGM_NO_VIEW2 0xFFFFFFFFu
fsgm_status fsgm_epi_plan_set_view2(fsgm_epi_plan* plan, int32_t on, int32_t direction);
fsgm_status fsgm_epi_plan_download_view2(fsgm_epi_plan* plan, int32_t frame, uint32_t* disp2, uint32_t* minC_v2);
/* Bytes of LDS a workgroup of the second view's kernel asks for at this dMax (1..1024; 0 above 256, the generic kernel), and the
 * second-view pixels a workgroup of the tiled kernel owns (0: the generic kernel, or a dMax out of range).  No device needed. */
fsgm_status fsgm_view2_launch_lds(int32_t dMax, uint64_t* bytes);
int32_t fsgm_view2_tile(int32_t dMax);

typedef struct {
    int32_t direction;         /* -1 or +1 */
    int32_t d_min;             /* |d_min| <= FSGM_D_MIN_LIMIT: candidate i stands for disparity d_min + i */
    int32_t max_diff;          /* >= 0, 1/256 units */
    int32_t reserved[5];       /* must be zero */
} fsgm_view2_params;
fsgm_view2_params fsgm_view2_params_default(void);   /* -1, 0, 256 */
/* sgm(C) with the second view: the arguments of fsgm_sgm_float_batch_host / _dptr without the format and with v2 (NULL: the
 * defaults) behind prm.  minC2 (not wanted) and S may be NULL, exact is a switch, exact with minC2 is FSGM_ERR_UNSUPPORTED.
 * disp2 u32 [n][H][W] is required; minC_v2 u32 and conf u8 [n][H][W] may be NULL.  agg_mode 2..6 is FSGM_ERR_UNSUPPORTED.  bestD,
 * minC, minC2 and S are those of the _ru, plain or _exact call, bit for bit.  The cached plan is never the plan of a call
 * without the second view.  Everything is refused before a device is touched; the _dptr form follows the device-pointer
 * contract (check table, caller's stream, status word, a captured stream refused) and writes disp2, minC_v2, conf where they lie. */
fsgm_status fsgm_sgm_view2_batch_host(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_sgm_params* prm, const fsgm_view2_params* v2, const uint8_t* guide,
                                      uint32_t* bestD, uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact, uint32_t* disp2,
                                      uint32_t* minC_v2, uint8_t* conf);
fsgm_status fsgm_sgm_view2_dptr(int32_t n_frames, const uint8_t* C, int32_t width, int32_t height, int32_t dMax, int32_t P1, int32_t P2,
                                const fsgm_sgm_params* prm, const fsgm_view2_params* v2, const uint8_t* guide, uint32_t* bestD,
                                uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact, uint32_t* disp2, uint32_t* minC_v2,
                                uint8_t* conf, void* stream, int32_t* status);
/* Rectified stereo with the second view: the arguments of fsgm_stereo_sgm_host_ru with minC2 nullable, plus max_diff; the
 * direction is prm's.  disp and disp2 (required) are int32 true disparities * 256, disp2's marker INT32_MIN; minC_v2 and conf may
 * be NULL.  prm->fb_check = 1 is FSGM_ERR_INVALID (that is the other door); there is no dMax <= 511 limit.  With prm->subpixel = 0
 * disp stays what the _range forms return, 256 * d_min + the whole index, while disp2 is 256 * (d_min + index): conf is computed on
 * d1 = 256 * (d_min + index), and fsgm_view2_check_* applies to such a pair only after the caller has scaled disp the same way. */
fsgm_status fsgm_stereo_sgm_view2_host(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                       int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt,
                                       int32_t d_min, int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf);
fsgm_status fsgm_stereo_sgm_view2_dptr(int32_t n_frames, const uint8_t* I1, const uint8_t* I2, int32_t width, int32_t height,
                                       int32_t dMax, int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt,
                                       int32_t d_min, int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf, void* stream, int32_t* status);
/* The check alone on int32 true-disparity maps [n][H][W] (disp2's marker INT32_MIN) -> conf u8 [n][H][W]; the status word of
 * the _dptr form is always 0. */
fsgm_status fsgm_view2_check_host(int32_t n_frames, const int32_t* disp, const int32_t* disp2, int32_t width, int32_t height,
                                  int32_t direction, int32_t max_diff, uint8_t* conf, int32_t device);
fsgm_status fsgm_view2_check_dptr(int32_t n_frames, const int32_t* disp, const int32_t* disp2, int32_t width, int32_t height,
                                  int32_t direction, int32_t max_diff, uint8_t* conf, int32_t device, void* stream, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FSGM_H */
