// capi_epi.hip -- C ABI for the calc_cost_sgm path: device-resident plan + host-pointer entry
// points (what the calc_cost_sgm mexFunction gateway calls).  See include/fsgm.h.
#include "capi_common.h"
#include "capi_device.h"
#include "capi_sgm.h"
#include "epi_kernels.h"
#include "epi_view2.h"
#include "geometry_kernels.h"
#include "post_kernels.h"
#include "post_plan.h"
#include "pyramid_kernels.h"
#include "sgm_ingest.h"
#include <algorithm>
#include <cmath>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace fsgm {
char* last_error_buf() {
    static thread_local char buf[512] = "";
    return buf;
}
}  // namespace fsgm

using namespace fsgm;

// What aggregates a plan's volumes: one member per pipeline (choose_pipeline), named by kPipelineName
enum Pipeline {
    PIPE_GENERIC, PIPE_PACKED_NOWRAP, PIPE_PACKED_WRAP,  // per-direction line kernels + WTA kernel
    PIPE_SWEEP,                                          // fused sweeps: horizontal pair, two frame lanes sweeping down then up
    PIPE_SWEEP_PAR,                                      // down and up sweeps side by side, WTA kernel over the three Y volumes
    PIPE_SWEEP_MID,                                      // as PIPE_SWEEP_PAR, the two sweeps meeting in the middle with the WTA inside
    PIPE_PAIRS,                                          // 4 paths: horizontal pair, vertical pair with the WTA inside
    PIPE_BAND,                                           // band sweeps: one workgroup per frame
    PIPE_BAND_CHAIN,                                     // band sweeps: one workgroup per (band, frame)
    PIPE_PACKED_EXACT, PIPE_GENERIC_EXACT,               // line kernels + WTA kernel with exact path arithmetic (fsgm_epi_plan_set_exact)
};
static const char* const kPipelineName[] = {"generic", "packed16/nowrap", "packed16/wrap", "sweep16/nowrap", "sweep16par/nowrap",
                                            "sweep16mid/nowrap", "pairs16/nowrap", "band16/nowrap", "band16chain/nowrap",
                                            "packed16/exact", "generic/exact"};
static bool pipe_exact(Pipeline k) { return k == PIPE_PACKED_EXACT || k == PIPE_GENERIC_EXACT; }
static bool pipe_lines(Pipeline k) { return k <= PIPE_PACKED_WRAP || pipe_exact(k); }
static bool pipe_sweep(Pipeline k) { return k == PIPE_SWEEP || k == PIPE_SWEEP_PAR || k == PIPE_SWEEP_MID; }

// The sub-forms of the selected pipeline, settled with it by select_kernel: decisions only, never device pointers (the
// device entry points swap some of the plan's for the length of one enqueue).
struct PipelineForm {
    int x_fine = 0;      // pairs, parallel sweeps: the along-x pair as pairx_* kernels (8 costs a lane), Y_h in natural d order
    int x_lines = 0;     // parallel sweeps: the along-x pair as two line-kernel slots instead (dLx)
    int tall = 0;        // parallel sweeps: 8-wave workgroups, half the launches of a sweep
    int mid_tall = 0;    // sweeps meeting in the middle: their final halves as 8-wave workgroups too
};

struct fsgm_epi_plan {
    int W = 0, H = 0, D = 0, batch = 0;
    fsgm_epi_params prm{};
    // How candidate d is sampled (fixed at creation): FSGM_SAMPLING_VZ at offset * vzInd(d) along the direction (the reference as
    // shipped), _LINEAR at d pixels along it (the reference built without USE_VZIND: the vz table holds d, the offsets 1.0),
    // _RECTIFIED a rectified pair -- Pd0 = (x + 1, y + 1), direction (direction, 0): no maps exist
    int sampling = FSGM_SAMPLING_VZ, direction = -1;
    int d_min = 0;                       // rectified: candidate index i stands for disparity d_min + i (fsgm_epi_plan_set_d_min)
    int P1 = 6, P2 = 64;                 // epipolar_sgm_of.m:19
    double vMax = 0.3;                   // epipolar_sgm_of.m:16
    size_t NP = 0, N = 0;                // pixels, voxels per frame
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *dI1 = nullptr, *dI2 = nullptr;
    uint32_t *dCen1 = nullptr, *dCen2 = nullptr;
    double *dPd0 = nullptr, *dNd = nullptr, *dOff = nullptr, *dVz = nullptr;
    double vzmax = 0.0;         // max |vzInd(d)| of the table in dVz (inf when not finite)
    uint8_t *dCraw = nullptr, *dC = nullptr, *dL = nullptr;
    uint32_t *dBestD = nullptr, *dMinC = nullptr, *dS = nullptr;
    uint32_t *dD2enc = nullptr, *dD2 = nullptr;          // forward-backward check (prm.fb_check)
    uint8_t* dConf = nullptr;
    // fused-sweep aggregation (epi_sweep.hip): horizontal path costs, u16 sums, block-boundary states
    // (see agg_sweep(): horizontal kernel on stream_h; the frames split into two lanes that sweep
    // down then up on stream / stream_b)
    uint8_t *dLh = nullptr, *dX = nullptr, *dXup = nullptr, *dState = nullptr, *dCkpt = nullptr, *dCkptV = nullptr;
    // parallel sweeps: Y_up of every frame and the up sweep's own block-boundary states
    uint8_t *dXupAll = nullptr, *dStateUp = nullptr;
    uint8_t* dLx = nullptr;              // parallel sweeps of few frames: the two along-x path volumes [batch][2][N] (form.x_lines)
    // band sweeps (epi_band.hip): the first pass's 9th bits, the hand-off between the bands of a frame; dX, dRec, dS0 as above
    uint32_t* dBits = nullptr;
    uint4* dBandEdge = nullptr;
    size_t band_edge_maps = 0;           // hand-off maps per frame the buffer holds (1: bands in sequence; bands - 1: chained)
    uint32_t *dBandTicket = nullptr, *dBandErr = nullptr;   // chained band sweeps: work counter, give-up flag of the bounded waits
    uint32_t band_salt = 0;              // launch sequence number of the chained form (hand-off tags)
    bool band_edge_untagged = false;     // the hand-off maps hold words without this scheme's tags (sequential form, S tap): refill before a chained launch
    // epipolar driver (fsgm_epipolar_sgm_of_host): rotation flow, composed flow, RGB staging
    double *dRflow = nullptr, *dFlow = nullptr;
    uint8_t* dRgb = nullptr;
    // test.m's frame body (fsgm_epipolar_flow_pp_*): the vz-index map, the host form's flow2, the chain's scratch plan
    double *dD1 = nullptr, *dFlow2 = nullptr;
    fsgm_post_plan* post = nullptr;
    uint2* dRec = nullptr;
    uint16_t* dS0 = nullptr;
    // caller-supplied volumes (fsgm_sgm_batch_host / fsgm_sgm_device): the host form's staging of [D][H][W] volumes, the flag
    // the ingest kernel raises for a byte above the declared bound
    uint8_t* dIngest = nullptr;
    uint32_t* dIngestFlag = nullptr;
    hipStream_t stream_h = nullptr, stream_b = nullptr;
    hipEvent_t ev_fork = nullptr, ev_h = nullptr, ev_b = nullptr, ev_c = nullptr;
    hipEvent_t ev_hl[2] = {nullptr, nullptr};   // the horizontal pair of each frame lane done (sweep pipeline)
    std::vector<int> cmax;               // per frame: upper bound of the cost values in dC
    bool vz_valid = false;
    int adaptive = 0;                    // adaptive P2 (calc_cost_sgm.cpp:68-72): line kernels at every batch size, the aggregation reads dI1
    std::vector<char> have_img;          // per frame: its image pair has been put into dI1 / dI2 (what an adaptive aggregation reads)
    int runner_up = 0;                   // the WTA also writes the runner-up cost (fsgm_epi_plan_set_runner_up): line kernels at every batch size
    uint32_t* dMinC2 = nullptr;          // [batch][NP], created when the switch first goes on
    int exact = 0;                       // exact path arithmetic (fsgm_epi_plan_set_exact): line kernels at every batch size, never with runner_up
    // second view (fsgm_epi_plan_set_view2): a WTA over the diagonal of S after the first view's, on the same volumes: line kernels at
    // every batch size.  v2_dir: candidate i of first-view pixel x is second-view pixel x + v2_dir * (d_min + i)
    int view2 = 0, v2_dir = -1;
    uint32_t *dDisp2v = nullptr, *dMinCv2 = nullptr;   // [batch][NP] each, created when the switch first goes on
    uint8_t* dConfV2 = nullptr;          // [batch][NP] the one-shot entries' left-right check, created on first use
    uint32_t v2_add = 0, v2_marker = 0xFFFFFFFFu;   // the stereo one-shot entries: 256 * d_min and INT32_MIN for the length of a call
    int agg_mode = 0;                    // 0 auto, 1 per-direction line kernels, 2 fused sweeps (if eligible), 3 parallel sweeps, 4 / 5 band sweeps, 6 sweeps meeting in the middle
    int cus = 256;                       // compute units of the device (band sweeps: one workgroup per frame, two per CU)
    Pipeline pipe = PIPE_GENERIC;
    PipelineForm form;
    DeviceJoin join;                     // device-pointer entry points: the events that order the plan's stream with the caller's
    bool pinned = false;                 // a captured graph names this cached plan's buffers, stream and events: never evicted (PlanCache)
};

// batch sizes at which auto mode moves from the line kernels to the parallel sweeps and on to the full sweep pipeline
// (8 paths; measured at 1242x375x128); FSGM_EPI_PAR_MIN / FSGM_EPI_PAR_MAX override them
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return (e && *e) ? atoi(e) : dflt; }
// The switch points were measured at 1242x375x128.  A fused pipeline's fixed latency goes with a linear dimension of the
// frame and the line kernels' time per frame with its voxels, so the batch at which the two cross goes with
// voxels^(-2/3): 320x240x64 (BASELINE configs[1], 1/12 of the voxels) measured ~26 / ~80 / ~48 frames for the three switches
// against 4 / 18 / 9 at the KITTI shape (profiles/r03_crossover_320x240x64.txt); the scaled values are 21 / 95 / 47.
// An environment override is taken as it stands.  FSGM_EPI_SHAPE_SCALE=0: the KITTI values for every shape.
static int scaled_batch(int W, int H, int D, int at_kitti) {
    static const int on = env_int("FSGM_EPI_SHAPE_SCALE", 1);
    if (!on) return at_kitti;
    const double s = std::pow(1242.0 * 375.0 * 128.0 / ((double)W * H * D), 2.0 / 3.0);
    return std::max(1, (int)std::lround(at_kitti * s));
}
static int switch_batch(const char* env_name, int W, int H, int D, int at_kitti) {
    const int e = env_int(env_name, -1);
    return e >= 0 ? e : scaled_batch(W, H, D, at_kitti);
}
static int par_min_batch(int W, int H, int D) { return switch_batch("FSGM_EPI_PAR_MIN", W, H, D, 4); }
static int par_max_batch(int W, int H, int D) { return switch_batch("FSGM_EPI_PAR_MAX", W, H, D, 26); }
// from this batch on the parallel sweeps meet in the middle (mode 6; profiles/r04_sweep_mid.txt: 10 frames 1.38 vs 1.44 ms, 18 frames
// 2.06 vs 2.41 -- and 2.61 for the full pipeline --, 28 frames 3.49 vs 3.35 for the full pipeline); FSGM_EPI_MID_MIN=0: never
static int mid_min_batch(int W, int H, int D) { return switch_batch("FSGM_EPI_MID_MIN", W, H, D, 10); }
// Band sweeps (all four paths of a pass in one sweep, one workgroup per frame, two workgroups per CU) in auto mode: a launch
// takes as long as its slowest CU -- measured at 1242x375x128, 8 paths, 256 CUs: 25.2 ms with one workgroup per CU (up to
// 256 frames), 42.8 ms with two (up to 512) -- while the block sweeps take 0.107 ms per frame whatever the count.  In units of
// the block sweeps' time per frame a round of the band kernel costs 0.92 x CUs (half filled) or 0.785 x 2 CUs (full): auto
// mode takes the band sweeps where that is less than the batch (256 frames, 402..512, 638..768, ...).
// FSGM_EPI_BAND_MIN: never below this many frames (0: never at all).
static int band_min_batch() { static const int v = env_int("FSGM_EPI_BAND_MIN", 64); return v; }
// (4 paths, against the pair pipeline's 0.084 ms per frame: 17.0 / 29.0 ms per round -> 0.74 x CUs / 0.63 x 2 CUs)
// The chained form (one workgroup per band and frame, mode 5) has no rounds: measured 7 ms + 0.076 ms per frame at 8 paths
// (profiles/r03_band_chain.txt: 96 .. 512 frames) = 0.26 x CUs + 0.71 per frame in the same units (4 paths: 0.23 x CUs + 0.68);
// it takes the batches between the sequential form's rounds (257 .. ~470 frames, 513 .. ~700, ...).
// Returns 0: neither pays, 1: sequential band sweeps, 2: chained.
// Other shapes: a band workgroup walks nbands x (W + skew x R) steps of R rows for H x W pixels (skew 2 with the diagonals,
// 1 without), the block sweeps' time goes with H x W: the costs above are scaled by that ratio relative to the KITTI shape
// (6 bands of 64 rows, 1242 columns).  320x240x64: a round measured 1.18 x 2 CUs (8 paths) and 0.90 x 2 CUs (4 paths) against
// 0.785 / 0.63 at the KITTI shape; the ratio gives 1.33 / 0.88 -- the band sweeps never pay there at 8 paths, from 512 frames at 4.
static double band_shape_cost(int W, int H, int D, int paths) {
    const int skew = paths == 8 ? 2 : 1;
    auto eff = [&](double w, double h, int R) { const int nb = ((int)h + R - 1) / R; return (h / (nb * R)) * (w / (w + skew * R)); };
    return eff(1242.0, 375.0, 64) / eff((double)W, (double)H, band_rows(D));
}
static int band_choice(int batch, int cus, int paths, int W, int H, int D) {
    if (band_min_batch() <= 0 || batch < band_min_batch()) return 0;
    const double g = band_shape_cost(W, H, D, paths);
    const double half = g * (paths == 8 ? 0.92 : 0.74), whole = g * (paths == 8 ? 0.785 : 0.63);
    const int slots = 2 * cus, full = batch / slots, tail = batch % slots;
    const double seq = full * whole * slots + (tail == 0 ? 0.0 : (tail <= cus ? half * cus : whole * slots));
    static const int chain_ok = env_int("FSGM_EPI_BAND_CHAIN", 1);                      // 0: auto mode never takes the chained form
    const double chain = chain_ok ? g * ((paths == 8 ? 0.26 : 0.23) * cus + (paths == 8 ? 0.71 : 0.68) * batch) : 1e30;
    if (std::min(seq, chain) >= (double)batch) return 0;
    return seq <= chain ? 1 : 2;
}
static int pairs_min_batch(int W, int H, int D) { return switch_batch("FSGM_EPI_PAIRS_MIN", W, H, D, 9); }   // 4 paths: line kernels -> pair pipeline

// What runs for a plan of this shape, batch and parameter set (cm: the largest cost in the volumes): a function of its
// arguments and the FSGM_EPI_* environment only, so that fsgm_epi_auto_pipeline can answer without a plan.
// adaptive: the plan's adaptive-P2 or runner-up switch is on -- either keeps it on the line kernels.
// exact: the plan's exact switch is on -- the line kernels that do not narrow, whatever the costs and penalties.
static Pipeline choose_pipeline(int W, int H, int D, int batch, int paths, int P1, int P2, int cm, int agg_mode, int cus,
                                int adaptive = 0, int exact = 0) {
    if (exact) return agg_line_split(D) ? PIPE_PACKED_EXACT : PIPE_GENERIC_EXACT;   // no fused pipeline carries 9-bit path costs
    if (!agg_line_split(D)) return PIPE_GENERIC;
    // (adaptive P2 lowers P2 per step, never raises it: the no-wrap test with the full P2 covers every step)
    const bool nowrap = P1 >= 0 && P2 >= 0 && cm + P2 + std::max(P1, P2) <= 255;
    Pipeline c = nowrap ? PIPE_PACKED_NOWRAP : PIPE_PACKED_WRAP;
    if (adaptive) return c;                                      // the fused pipelines have no per-step P2 (and their WTA tails no second minimum): line kernels at every batch size
    // 48 .. 224 (12, 20 or 28 costs a lane): the fused pipelines' register layout is 16 costs a lane -- line kernels at every
    // batch size and under every forced mode, as for a dMax the generic kernels take
    if (agg_packed_lpp(D) == 0) return c;
    // the fused sweeps cover the 8-path no-wrap case; everything else stays on the line kernels
    // Auto mode takes the fused pipelines only for batches: their latency (H rows in sequence for a sweep, down then
    // up; three passes along 1242-pixel rows for a pair) is 1.0 / 2.0 ms (4 / 8 paths) whatever the frame count,
    // while the line kernels scale with it.  Measured at 1242x375x128 (ms per batch, line vs fused):
    // 8 paths 8 frames 1.96 / 2.20, 12 frames 2.89 / 2.29; 4 paths 8 frames 1.18 / 1.19, 12 frames 1.67 / 1.28.
    const int min_batch = paths == 8 ? par_min_batch(W, H, D) : pairs_min_batch(W, H, D);
    const bool want = agg_mode == 2 || agg_mode == 3 || agg_mode == 6 || (agg_mode == 0 && batch >= min_batch);
    // (P1 <= P2: the fused kernels' form of the step clamps path states at P2 first, epi_sweep.hip)
    const bool fusable = nowrap && P1 <= P2;
    // (the Y volumes hold y + P1 per path since round 3 -- step_b, epi_step.h -- so three / two of them must fit a byte with the bias)
    if (fusable && 3 * (P1 + P2) <= 255 && paths == 8 && want) {
        // Between the line kernels and the full pipeline: the down and the up sweep side by side (H rows in sequence
        // instead of 2 H) with Y_up written out and a WTA kernel over C, Y_dn, Y_up, Y_h: 3 B per voxel more traffic,
        // half the latency.  Mode 3 forces it; auto takes it while the batch is too small to hide the longer chain.
        const bool par = agg_mode == 3 || agg_mode == 6 || (agg_mode == 0 && batch < par_max_batch(W, H, D));
        // Mode 6, and auto for the larger of the batches that take the parallel sweeps: the two sweeps meet in the middle.  Each
        // writes its Y for its first half of the rows only and crosses the other's half as a final sweep (the other's Y, Y_h,
        // WTA in registers): the traffic of the full pipeline (9.6 B per voxel measured, no WTA kernel over four volumes) on the
        // parallel sweeps' chain of H rows.
        const int mid_min = mid_min_batch(W, H, D);
        const bool mid = agg_mode == 6 || (agg_mode == 0 && par && mid_min > 0 && batch >= mid_min);
        c = mid ? PIPE_SWEEP_MID : par ? PIPE_SWEEP_PAR : PIPE_SWEEP;
    }
    // the shipped 4-path configuration: both axes as pair kernels, the vertical one final
    if (fusable && 2 * (P1 + P2) <= 255 && paths == 4 && want) c = PIPE_PAIRS;
    // very large batches (or mode 4 / 5): the band sweeps
    const int band = agg_mode == 0 ? band_choice(batch, cus, paths, W, H, D) : 0;
    if (fusable && band_ok(D, paths, P1, P2, cm) && (agg_mode == 4 || agg_mode == 5 || band != 0)) {
        // mode 5 / auto between the sequential form's rounds: the bands of a frame as workgroups of their own (chained)
        c = agg_mode == 5 || band == 2 ? PIPE_BAND_CHAIN : PIPE_BAND;
    }
    return c;
}

// The pipeline and its sub-forms, settled together: enqueue() and the S tap read them and re-derive nothing.  The sub-form
// switches (A/B) are read here, once per process.
static void select_kernel(fsgm_epi_plan* p) {
    const int cm = *std::max_element(p->cmax.begin(), p->cmax.end());
    const Pipeline k = choose_pipeline(p->W, p->H, p->D, p->batch, p->prm.paths, p->P1, p->P2, cm, p->agg_mode, p->cus,
                                       p->adaptive || p->runner_up || p->view2, p->exact);
    const int B = p->batch;
    const bool fine_ok = pair_x_fine_ok(p->D) != 0;
    PipelineForm f;
    // 4-path pipeline: the along-x pair as pairx_* kernels (8 costs a lane).  Small batches wait for that pair's serial chain,
    // which the finer split shortens (2 / 9 frames at 1242x375x128: 0.96 -> 0.82 / 1.24 -> 1.12 ms); from 16 frames the
    // pipeline is bound by its HBM traffic (7.5 B per voxel at ~5 TB/s) and the coarser kernels' fewer instructions win
    // (40 frames: 3.47 against 3.68 ms).  FSGM_PAIR_XFINE=0 / 1: never / always (A/B switch).
    static const int pair_xfine = env_int("FSGM_PAIR_XFINE", -1);
    if (k == PIPE_PAIRS) f.x_fine = fine_ok && pair_xfine != 0 && (pair_xfine == 1 || B < 16);
    // Parallel sweeps (8 paths, 5..17 frames): what the batch waits for are serial chains -- the along-x pair's 3 x W steps and
    // the sweeps' H / 16 launches.  FSGM_EPI_PAR_FINE / FSGM_EPI_PAR_TALL = 0 / 1 force the two shortenings off / on (A/B).
    static const int par_fine = env_int("FSGM_EPI_PAR_FINE", -1), par_tall = env_int("FSGM_EPI_PAR_TALL", -1);
    if (k == PIPE_SWEEP_PAR || k == PIPE_SWEEP_MID) {
        f.x_fine = fine_ok && par_fine != 0 && (par_fine == 1 || B <= 10);   // 8 frames 1.46 -> 1.32 ms with both; from 12 frames neither pays
        f.tall = par_tall >= 0 ? par_tall != 0 : B <= 10;
    }
    // Parallel sweeps (not the form that meets in the middle, whose final sweeps read Y_h): the along-x pair as two line-kernel slots.
    // FSGM_EPI_PAR_XLINES: 0 never, 1 whenever possible; default: up to 5 frames -- 4 frames 0.871 -> 0.832 ms, 6 frames 0.970 -> 1.050:
    // with more frames the two volumes' bytes and the lines' instructions cost more than the pair's longer chain
    // (profiles/r04_par_xlines.txt).
    static const int xlines = env_int("FSGM_EPI_PAR_XLINES", -1);
    if (k == PIPE_SWEEP_PAR) f.x_lines = xlines != 0 && (xlines == 1 || B <= 5);
    // the final halves of the sweeps that meet in the middle as 8-wave workgroups too (FSGM_EPI_MID_TALL: A/B switch)
    static const int mid_tall = env_int("FSGM_EPI_MID_TALL", -1);
    if (k == PIPE_SWEEP_MID) f.mid_tall = mid_tall >= 0 ? mid_tall != 0 : f.tall;
    p->pipe = k;
    p->form = f;
}

// Lazily created buffer sets.  Everything is created aside and committed to the plan only when the whole set exists, so
// a failure midway leaves the plan as it was (nothing leaked, nothing half-initialised for the next call to trip over).
namespace {
struct LazySet {
    struct Item { void** slot; void* v; int kind; };     // kind 0: buffer, 1: stream, 2: event
    std::vector<Item> items;
    hipError_t err = hipSuccess;
    // a buffer for `slot` when wanted and the slot is empty (or to replace it); returns it, null when none was created
    template <class T> T* alloc(T*& slot, size_t bytes, bool want = true, bool replace = false) {
        if (!want || (slot && !replace) || err != hipSuccess) return nullptr;
        void* v = nullptr;
        err = hipMalloc(&v, bytes ? bytes : 1);
        if (err != hipSuccess) return nullptr;
        items.push_back({(void**)&slot, v, 0});
        return (T*)v;
    }
    void stream(hipStream_t& slot, bool want = true) {
        hipStream_t s = nullptr;
        if (!want || slot || err != hipSuccess) return;
        if ((err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) == hipSuccess) items.push_back({(void**)&slot, s, 1});
    }
    void event(hipEvent_t& slot, bool want = true) {
        hipEvent_t e = nullptr;
        if (!want || slot || err != hipSuccess) return;
        if ((err = hipEventCreateWithFlags(&e, hipEventDisableTiming)) == hipSuccess) items.push_back({(void**)&slot, e, 2});
    }
    void commit() {
        for (Item& i : items) *i.slot = i.v;
    }
    void rollback() {
        for (Item& i : items)
            if (i.kind == 0) (void)hipFree(i.v);
            else if (i.kind == 1) (void)hipStreamDestroy((hipStream_t)i.v);
            else (void)hipEventDestroy((hipEvent_t)i.v);
    }
};
fsgm_status lazy_fail(LazySet& ls, const char* what) {
    ls.rollback();
    return hip_status(ls.err, what);
}
// frame offset into a buffer the selected pipeline may not have
template <class T> T* frame_at(T* base, size_t off) { return base ? base + off : nullptr; }
}  // namespace

extern "C" {

const char* fsgm_last_error(void) { return last_error_buf(); }

int fsgm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

fsgm_status fsgm_device_arch(int device, char* buf, size_t buflen) {
    FSGM_REQUIRE(buf && buflen > 0, "fsgm_device_arch: null buffer");
    hipDeviceProp_t prop;
    FSGM_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buflen, "%s", prop.gcnArchName);
    return FSGM_OK;
}

fsgm_epi_params fsgm_epi_params_default(void) {
    fsgm_epi_params p;
    p.paths = 4;         // calc_cost_sgm.cpp:104
    p.subpixel = 1;      // calc_cost_sgm.cpp:560
    p.vz_to_disp = 1;    // calc_cost_sgm.cpp:4
    p.device = 0;
    p.fb_check = 0;      // calc_cost_sgm.cpp:589-590 (commented out)
    return p;
}

void fsgm_epi_plan_destroy(fsgm_epi_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->prm.device);
    // An evicted plan may still have device-form work queued (PlanCache::insert): drain it before anything is freed, not by
    // way of what hipFree happens to wait for.
    for (hipStream_t st : {p->stream, p->stream_h, p->stream_b})
        if (st) (void)hipStreamSynchronize(st);
    void* bufs[] = {p->dI1, p->dI2, p->dCen1, p->dCen2, p->dPd0, p->dNd, p->dOff, p->dVz,
                    p->dCraw, p->dC, p->dL, p->dBestD, p->dMinC, p->dS, p->dD2enc, p->dD2, p->dConf, p->dLh, p->dX, p->dXup, p->dXupAll, p->dStateUp, p->dLx, p->dState, p->dCkpt, p->dCkptV, p->dRec, p->dS0, p->dRflow, p->dFlow, p->dRgb, p->dBits, p->dBandEdge, p->dBandTicket, p->dBandErr,
                    p->dD1, p->dFlow2, p->dIngest, p->dIngestFlag, p->dMinC2, p->dDisp2v, p->dMinCv2, p->dConfV2};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    fsgm_post_plan_destroy(p->post);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    for (hipEvent_t e : {p->ev_fork, p->ev_h, p->ev_b, p->ev_c, p->ev_hl[0], p->ev_hl[1]})
        if (e) (void)hipEventDestroy(e);
    p->join.destroy();
    for (hipStream_t st : {p->stream, p->stream_h, p->stream_b})
        if (st) (void)hipStreamDestroy(st);
    delete p;
}

fsgm_status fsgm_epi_plan_create(fsgm_epi_plan** out, int32_t W, int32_t H, int32_t D, int32_t batch,
                                 const fsgm_epi_params* prm) {
    return fsgm_epi_plan_create_sampling(out, W, H, D, batch, prm, FSGM_SAMPLING_VZ, 0);
}

// what a plan can be refused for without a GPU (pr: vz_to_disp already cleared for the samplings that have none); the device
// entry points that run on a cached plan ask this before they touch a device, as plan creation does
static fsgm_status epi_plan_args(int W, int H, int D, int batch, const fsgm_epi_params& pr, int sampling, int direction) {
    FSGM_REQUIRE(sampling == FSGM_SAMPLING_VZ || sampling == FSGM_SAMPLING_LINEAR || sampling == FSGM_SAMPLING_RECTIFIED,
                 "fsgm_epi_plan_create: sampling must be FSGM_SAMPLING_VZ, _LINEAR or _RECTIFIED (got %d)", sampling);
    FSGM_REQUIRE(sampling != FSGM_SAMPLING_RECTIFIED || direction == -1 || direction == 1,
                 "fsgm_epi_plan_create: a rectified plan's direction must be -1 or +1 (got %d)", direction);
    FSGM_REQUIRE(W >= 1 && H >= 1, "fsgm_epi_plan_create: width/height must be >= 1 (got %d x %d)", W, H);
    FSGM_REQUIRE(D >= 1, "fsgm_epi_plan_create: dMax must be >= 1 (got %d)", D);
    FSGM_REQUIRE(batch >= 1, "fsgm_epi_plan_create: batch must be >= 1");
    // (the line, census, cost, WTA and sweep kernels take the frame as blockIdx.y / .z)
    if (batch > 65535) return fail(FSGM_ERR_UNSUPPORTED, "fsgm_epi_plan_create: batch %d exceeds 65535 frames (the frame is a grid dimension)", batch);
    FSGM_REQUIRE(pr.paths == 4 || pr.paths == 8, "fsgm_epi_plan_create: paths must be 4 or 8 (got %d)", pr.paths);
    if (pr.fb_check && D > 511)
        return fail(FSGM_ERR_UNSUPPORTED, "fb_check needs dMax <= 511 (bestD must stay below INVALID_DISPARITY)");
    if (D > FSGM_GENERIC_MAX_D)
        return fail(FSGM_ERR_UNSUPPORTED, "dMax %d exceeds the supported maximum %d", D, FSGM_GENERIC_MAX_D);
    if ((double)W * H * D >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "cost volume %d x %d x %d exceeds 2^31 voxels per frame", W, H, D);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_create_sampling(fsgm_epi_plan** out, int32_t W, int32_t H, int32_t D, int32_t batch,
                                          const fsgm_epi_params* prm, int32_t sampling, int32_t direction) {
    FSGM_REQUIRE(out, "fsgm_epi_plan_create: null plan pointer");
    *out = nullptr;
    fsgm_epi_params pr = prm ? *prm : fsgm_epi_params_default();
    if (sampling != FSGM_SAMPLING_VZ) pr.vz_to_disp = 0;         // bestD is the index * 256, never converted (:592-594)
    { const fsgm_status as = epi_plan_args(W, H, D, batch, pr, sampling, direction); if (as != FSGM_OK) return as; }
    { const fsgm_status ds = use_device(pr.device); if (ds != FSGM_OK) return ds; }

    fsgm_epi_plan* p = new fsgm_epi_plan;
    p->W = W; p->H = H; p->D = D; p->batch = batch; p->prm = pr;
    p->sampling = sampling; p->direction = sampling == FSGM_SAMPLING_RECTIFIED ? direction : 0;
    const bool rect = sampling == FSGM_SAMPLING_RECTIFIED;
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, pr.device) == hipSuccess && n > 0) p->cus = n; }
    p->NP = (size_t)W * H; p->N = p->NP * D;
    p->cmax.assign(batch, 24);           // census 5x5: 24 informative bits
    p->have_img.assign(batch, 0);
    const size_t B = batch;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** ptr, size_t bytes) { if (e == hipSuccess) e = hipMalloc(ptr, bytes); };
    // images, census codes, the two fp64 coordinate maps and the raw cost volume belong to the cost stage and are allocated
    // on first use (ensure_cost_buffers): an aggregation-only plan holds C, the offsets and its pipeline's volumes only
    if (!rect) alloc((void**)&p->dOff, B * p->NP * 8);           // (a rectified plan has no maps)
    alloc((void**)&p->dVz, (size_t)D * 8);
    alloc((void**)&p->dC, B * p->N);
    // the per-voxel intermediates of the two aggregation strategies (L_r for the line kernels;
    // L_left/right, X_dn, states, records for the fused sweeps) are allocated on first use
    alloc((void**)&p->dBestD, B * p->NP * 4);
    alloc((void**)&p->dMinC, B * p->NP * 4);
    if (pr.fb_check) {
        alloc((void**)&p->dD2enc, B * p->NP * 4);
        alloc((void**)&p->dD2, B * p->NP * 4);
        alloc((void**)&p->dConf, B * p->NP);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e == hipSuccess && sampling == FSGM_SAMPLING_VZ) e = hipMemsetAsync(p->dOff, 0, B * p->NP * 8, p->stream);
    if (e == hipSuccess && sampling == FSGM_SAMPLING_LINEAR) {   // offset == 1.0 for good: (1.0 * d) * u is the reference's d * u (:368-369)
        const std::vector<double> ones(B * p->NP, 1.0);
        e = hipMemcpy(p->dOff, ones.data(), B * p->NP * 8, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        fsgm_epi_plan_destroy(p);
        return hip_status(e, "fsgm_epi_plan_create");
    }
    // once per device: the fused kernels' packed 3-input max / min must be exact u16 operations (epi_sweep.hip)
    {
        static std::mutex mu;
        static int state[64] = {0};                          // 0 unknown, 1 good, 2 bad
        std::lock_guard<std::mutex> lk(mu);
        int& s = state[pr.device & 63];
        if (s == 0) {
            int r = fused_step_selftest(p->stream);
            if (r == 0) r = costbox_selftest(p->stream);         // the fused cost kernel's mean as one fp16 multiply on denormal patterns
            if (r < 0) { fsgm_epi_plan_destroy(p); return fail(FSGM_ERR_HIP, "fsgm_epi_plan_create: self-test of the packed step could not run"); }
            s = r == 0 ? 1 : 2;
        }
        if (s == 2) {
            fsgm_epi_plan_destroy(p);
            return fail(FSGM_ERR_UNSUPPORTED, "this build's v_pk_maximum3_f16 / v_pk_minimum3_f16 / v_pk_mul_f16 do not act as exact u16 operations on denormal "
                                              "patterns (toolchain or float-mode change): the fused kernels would be wrong");
        }
    }
    select_kernel(p);
    *out = p;
    return FSGM_OK;
}

// Buffers of the cost stage (census x2 -> raw costs -> box mean) and of everything else that reads the image pair or the
// coordinate maps: created together on first use, committed only when the whole set exists.
static fsgm_status ensure_cost_buffers(fsgm_epi_plan* p) {
    if (p->dCraw) return FSGM_OK;                                // the set's own marker: created last
    const size_t B = p->batch;
    LazySet ls;
    ls.alloc(p->dI1, B * p->NP);                                 // (a slot that is filled already stays: ensure_image_buffers)
    ls.alloc(p->dI2, B * p->NP);
    ls.alloc(p->dCen1, B * p->NP * 4);
    ls.alloc(p->dCen2, B * p->NP * 4);
    ls.alloc(p->dPd0, B * p->NP * 16, p->sampling != FSGM_SAMPLING_RECTIFIED);
    ls.alloc(p->dNd, B * p->NP * 16, p->sampling != FSGM_SAMPLING_RECTIFIED);
    ls.alloc(p->dCraw, B * p->N);
    if (ls.err != hipSuccess) return lazy_fail(ls, "cost stage buffers");
    ls.commit();
    return FSGM_OK;
}

// The image pair alone: what fsgm_epi_plan_upload_images fills.  An aggregation-only plan with adaptive P2 holds these and
// none of the cost stage's other buffers.
static fsgm_status ensure_image_buffers(fsgm_epi_plan* p) {
    if (p->dI1 && p->dI2) return FSGM_OK;
    LazySet ls;
    ls.alloc(p->dI1, (size_t)p->batch * p->NP);
    ls.alloc(p->dI2, (size_t)p->batch * p->NP);
    if (ls.err != hipSuccess) return lazy_fail(ls, "image buffers");
    ls.commit();
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_penalties(fsgm_epi_plan* p, int32_t P1, int32_t P2, double vMax) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(!p->exact || (P1 >= 0 && P1 <= 255 && P2 >= 0 && P2 <= 255),
                 "fsgm_epi_plan_set_penalties: an exact plan takes P1 and P2 in 0..255 (got %d, %d)", P1, P2);
    p->P1 = P1; p->P2 = P2;
    if (vMax != p->vMax) p->vz_valid = false;
    p->vMax = vMax;
    select_kernel(p);
    return FSGM_OK;
}

static fsgm_status ensure_vz(fsgm_epi_plan* p) {
    if (p->vz_valid) return FSGM_OK;
    // calc_cost_sgm.cpp:339,360-361 -- depends on d only; same fp64 expressions, host side
    std::vector<double> vz(p->D);
    double vzmax = 0.0;
    const double n = p->D + 1;
    for (int d = 0; d < p->D; d++) {
        const double vzRatio = 1.0 * d / n * p->vMax;
        vz[d] = p->sampling == FSGM_SAMPLING_VZ ? vzRatio / (1 - vzRatio) : (double)d;   // linear: d itself (:368-369)
        vzmax = std::isfinite(vz[d]) ? std::max(vzmax, std::fabs(vz[d])) : INFINITY;
    }
    FSGM_HIP(hipMemcpyAsync(p->dVz, vz.data(), (size_t)p->D * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));   // vz is a stack-lifetime host buffer
    p->vzmax = vzmax;
    p->vz_valid = true;
    return FSGM_OK;
}

// the chained band sweeps' bounded hand-off waits raise a device flag instead of hanging: surface it after a sync
static fsgm_status check_handoff(fsgm_epi_plan* p) {
    if (p->dBandErr) {                                           // a chained launch happened at some point (the selection may have moved on since)
        uint32_t e = 0;
        FSGM_HIP(hipMemcpy(&e, p->dBandErr, sizeof(e), hipMemcpyDeviceToHost));
        if (e != 0) {
            (void)hipMemset(p->dBandErr, 0, sizeof(e));
            return fail(FSGM_ERR_HIP, "band sweep: a hand-off between the bands of a frame timed out (results of this run are invalid)");
        }
    }
    return FSGM_OK;
}

// An entry point's frame f: in range, the device current, and (drain 1) the plan's stream drained, (drain 2) with the chained
// band sweeps' hand-off flag checked
static fsgm_status frame_ready(fsgm_epi_plan* p, int f, int drain) {
    FSGM_REQUIRE(f >= 0 && f < p->batch, "frame %d out of range (batch %d)", f, p->batch);
    FSGM_HIP(hipSetDevice(p->prm.device));
    if (drain) FSGM_HIP(hipStreamSynchronize(p->stream));
    return drain == 2 ? check_handoff(p) : FSGM_OK;
}

// frame f's images and maps up on the plan's stream (the caller drains it before the host buffers may change)
static fsgm_status upload_async(fsgm_epi_plan* p, int f, const uint8_t* I1, const uint8_t* I2, const double* pd0, const double* nd,
                                const double* off) {
    const size_t NP = p->NP, o = (size_t)f;
    FSGM_HIP(hipMemcpyAsync(p->dI1 + o * NP, I1, NP, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dI2 + o * NP, I2, NP, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dPd0 + o * 2 * NP, pd0, NP * 16, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dNd + o * 2 * NP, nd, NP * 16, hipMemcpyHostToDevice, p->stream));
    if (p->sampling == FSGM_SAMPLING_VZ) FSGM_HIP(hipMemcpyAsync(p->dOff + o * NP, off, NP * 8, hipMemcpyHostToDevice, p->stream));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_upload(fsgm_epi_plan* p, int32_t f, const uint8_t* I1, const uint8_t* I2,
                                 const double* pd0, const double* nd, const double* off) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 0); if (fs != FSGM_OK) return fs; }
    FSGM_REQUIRE(p->sampling != FSGM_SAMPLING_RECTIFIED, "fsgm_epi_plan_upload: a rectified plan takes images only (fsgm_epi_plan_upload_images)");
    FSGM_REQUIRE(I1 && I2 && pd0 && nd && (off || p->sampling == FSGM_SAMPLING_LINEAR), "fsgm_epi_plan_upload: null input");
    { fsgm_status cs = ensure_cost_buffers(p); if (cs != FSGM_OK) return cs; }
    StreamGuard guard(p->stream);
    { fsgm_status us = upload_async(p, f, I1, I2, pd0, nd, off); if (us != FSGM_OK) return us; }
    FSGM_HIP(hipStreamSynchronize(p->stream));   // pageable host memory: keep the caller's buffers free to reuse
    guard.dismiss();
    p->have_img[f] = 1;
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_upload_images(fsgm_epi_plan* p, int32_t f, const uint8_t* I1, const uint8_t* I2) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 0); if (fs != FSGM_OK) return fs; }
    FSGM_REQUIRE(I1 && I2, "fsgm_epi_plan_upload_images: null input");
    { fsgm_status cs = ensure_image_buffers(p); if (cs != FSGM_OK) return cs; }   // (the cost stage's other buffers: prepare())
    StreamGuard guard(p->stream);
    FSGM_HIP(hipMemcpyAsync(p->dI1 + (size_t)f * p->NP, I1, p->NP, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dI2 + (size_t)f * p->NP, I2, p->NP, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    p->have_img[f] = 1;
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_upload_cost(fsgm_epi_plan* p, int32_t f, const uint8_t* C) {
    FSGM_REQUIRE(p && C, "fsgm_epi_plan_upload_cost: null argument");
    { fsgm_status fs = frame_ready(p, f, 0); if (fs != FSGM_OK) return fs; }
    int cm = 0;
    for (size_t i = 0; i < p->N; i++) cm = C[i] > cm ? C[i] : cm;
    p->cmax[f] = cm;
    select_kernel(p);
    FSGM_HIP(hipMemcpyAsync(p->dC + f * p->N, C, p->N, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    return FSGM_OK;
}

// frame dst <- frame src of the resident cost volumes, columns rotated by roll_cols (dst[y][(x + roll) % W] = src[y][x]):
// how bench.py fills a large batch with distinct volumes without pushing each through PCIe
fsgm_status fsgm_epi_plan_copy_cost(fsgm_epi_plan* p, int32_t dst, int32_t src, int32_t roll_cols) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(dst >= 0 && dst < p->batch && src >= 0 && src < p->batch && dst != src, "fsgm_epi_plan_copy_cost: bad frame pair %d <- %d", dst, src);
    FSGM_HIP(hipSetDevice(p->prm.device));
    const size_t pitch = (size_t)p->W * p->D;
    const int s = ((roll_cols % p->W) + p->W) % p->W;
    uint8_t* d0 = p->dC + (size_t)dst * p->N;
    const uint8_t* s0 = p->dC + (size_t)src * p->N;
    if (s == 0) {
        FSGM_HIP(hipMemcpyAsync(d0, s0, p->N, hipMemcpyDeviceToDevice, p->stream));
    } else {
        FSGM_HIP(hipMemcpy2DAsync(d0 + (size_t)s * p->D, pitch, s0, pitch, (size_t)(p->W - s) * p->D, p->H, hipMemcpyDeviceToDevice, p->stream));
        FSGM_HIP(hipMemcpy2DAsync(d0, pitch, s0 + (size_t)(p->W - s) * p->D, pitch, (size_t)s * p->D, p->H, hipMemcpyDeviceToDevice, p->stream));
    }
    p->cmax[dst] = p->cmax[src];
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_upload_offset(fsgm_epi_plan* p, int32_t f, const double* off) {
    FSGM_REQUIRE(p && off, "fsgm_epi_plan_upload_offset: null argument");
    FSGM_REQUIRE(p->sampling == FSGM_SAMPLING_VZ, "fsgm_epi_plan_upload_offset: only vz-index plans have an offset map");
    { fsgm_status fs = frame_ready(p, f, 0); if (fs != FSGM_OK) return fs; }
    FSGM_HIP(hipMemcpyAsync(p->dOff + f * p->NP, off, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    return FSGM_OK;
}

// The buffers of the selected pipeline that are still missing, created together and committed only when all of them exist.
// The pipelines share some -- records, S[0] words, Y volumes, the pair's stream, the boundary states -- and a plan may be
// switched from one to another: only what is still missing is created.
static fsgm_status ensure_agg_buffers(fsgm_epi_plan* p) {
    const Pipeline k = p->pipe;
    const bool lines = pipe_lines(k), pairs = k == PIPE_PAIRS, sweep = pipe_sweep(k), band = k == PIPE_BAND || k == PIPE_BAND_CHAIN;
    const bool par = k == PIPE_SWEEP_PAR || k == PIPE_SWEEP_MID, chain = k == PIPE_BAND_CHAIN;
    const size_t B = p->batch, N = p->N, NP = p->NP, state_bytes = sweep_state_bytes(p->W, p->D);
    // band sweeps: one hand-off map per frame, one per band boundary in the chained form (the buffer only grows)
    const int R = band_rows(p->D);
    const size_t nbands = R ? (size_t)(p->H + R - 1) / R : 1;
    const size_t maps = chain ? (nbands > 1 ? nbands - 1 : 1) : 1;
    const bool new_edge = band && (!p->dBandEdge || p->band_edge_maps < maps);
    const size_t edge_bytes = B * maps * band_edge_uint4s(p->W, p->D, 8) * sizeof(uint4);
    LazySet ls;
    ls.alloc(p->dL, B * N * p->prm.paths, lines);
    ls.alloc(p->dLh, B * N, pairs || sweep);
    ls.alloc(p->dCkpt, B * pair_ckpt_bytes(p->W, p->H, p->D, 0), pairs || sweep);
    ls.alloc(p->dCkptV, B * pair_ckpt_bytes(p->W, p->H, p->D, 1), pairs);
    ls.alloc(p->dRec, B * NP * sizeof(uint2), !lines);
    ls.alloc(p->dS0, B * NP * sizeof(uint16_t), !lines);
    ls.alloc(p->dX, B * N, sweep || band);
    ls.alloc(p->dState, 2 * B * state_bytes, sweep);
    ls.alloc(p->dXupAll, B * N, par);
    ls.alloc(p->dStateUp, 2 * B * state_bytes, par);
    ls.alloc(p->dLx, 2 * B * N, p->form.x_lines != 0);
    uint4* edge = ls.alloc(p->dBandEdge, edge_bytes, new_edge, true);
    ls.alloc(p->dBits, B * band_bits_u32s(p->W, p->H, p->D) * sizeof(uint32_t), band && p->prm.paths == 8);
    ls.alloc(p->dBandTicket, sizeof(uint32_t), chain);
    uint32_t* err = ls.alloc(p->dBandErr, sizeof(uint32_t), chain);
    ls.stream(p->stream_h, pairs || sweep);
    ls.stream(p->stream_b, sweep);
    for (hipEvent_t* e : {&p->ev_fork, &p->ev_h}) ls.event(*e, pairs || sweep);
    for (hipEvent_t* e : {&p->ev_b, &p->ev_c, &p->ev_hl[0], &p->ev_hl[1]}) ls.event(*e, sweep);
    // chained form: hand-off dwords carry a launch tag in their bytes' top bits; all ones = "older than any launch"
    if (ls.err == hipSuccess && edge && chain) ls.err = hipMemsetAsync(edge, 0xFF, edge_bytes, p->stream);
    if (ls.err == hipSuccess && err) ls.err = hipMemsetAsync(err, 0, sizeof(uint32_t), p->stream);
    if (ls.err != hipSuccess) return lazy_fail(ls, "aggregation buffers");
    if (edge && p->dBandEdge) { (void)hipStreamSynchronize(p->stream); (void)hipFree(p->dBandEdge); }
    if (edge) { p->band_salt = 0; p->band_edge_maps = maps; }
    ls.commit();
    return FSGM_OK;
}

// What a run of `stages` needs before anything is queued: the cost stage rewrites C with census costs
// (values <= 24), so the bound of the cost values -- and with it the kernel selection -- is settled first;
// then the buffer set of the selected pipeline.
static fsgm_status prepare(fsgm_epi_plan* p, int stages) {
    if (p->adaptive && (stages & FSGM_STAGE_AGGREGATE)) {        // the aggregation reads I1 of every slot: refuse before anything is queued
        for (int f = 0; f < p->batch; f++)
            if (!p->dI1 || !p->have_img[f])
                return fail(FSGM_ERR_INVALID, "adaptive P2: no image uploaded for frame %d (fsgm_epi_plan_upload / _upload_images)", f);
    }
    if (p->view2 && (stages & FSGM_STAGE_COST) && p->sampling != FSGM_SAMPLING_RECTIFIED)
        return fail(FSGM_ERR_INVALID, "second view: the candidates of this plan's own cost stage share no line (upload the cost volumes instead)");
    if ((stages & FSGM_STAGE_COST) || p->prm.fb_check) {
        fsgm_status cs = ensure_cost_buffers(p);
        if (cs != FSGM_OK) return cs;
    }
    if (stages & FSGM_STAGE_COST) {
        bool changed = false;
        for (int& c : p->cmax) { if (c != 24) changed = true; c = 24; }
        if (changed) select_kernel(p);
    }
    if (stages & (FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) return ensure_agg_buffers(p);
    return FSGM_OK;
}

// Where the sweeps that meet in the middle meet: the row count of the down sweep's first half, a whole number of its launches
// (the up sweep's first half, H - hm rows, ends with a short launch).
static int meet_row(int H, int D) {
    const int t = 2 * sweep_rows_per_launch(D);                  // rows per launch of the 8-wave form
    const int hm = ((H + 1) / 2 + t - 1) / t * t;
    return std::min(hm, H);
}

// census x2 + cost fill + box of frames [f0, f0 + nf) on the plan's stream (ensure_vz done by the caller)
static void enqueue_cost(fsgm_epi_plan* p, int f0, int nf) {
    const size_t NP = p->NP, o = (size_t)f0;
    launch_census(p->stream, p->dI1 + o * NP, p->dCen1 + o * NP, p->W, p->H, nf);
    launch_census(p->stream, p->dI2 + o * NP, p->dCen2 + o * NP, p->W, p->H, nf);
    if (p->sampling == FSGM_SAMPLING_RECTIFIED) {
        launch_stereo_cost(p->stream, p->dCen1 + o * NP, p->dCen2 + o * NP, p->dCraw + o * p->N, p->dC + o * p->N, p->W, p->H, p->D,
                           p->direction, nf, p->d_min);
        return;
    }
    EpiCostArgs a;
    a.cen1 = p->dCen1 + o * NP; a.cen2 = p->dCen2 + o * NP; a.pd0 = p->dPd0 + o * 2 * NP; a.nd = p->dNd + o * 2 * NP;
    a.off = p->dOff + o * NP; a.vz = p->dVz; a.vzmax = p->vzmax; a.Craw = p->dCraw + o * p->N; a.W = p->W; a.H = p->H; a.D = p->D;
    launch_epi_cost(p->stream, a, p->dC + o * p->N, nf);
}

// ---- launch arguments from frame f0 on.  They read the plan's buffer pointers when called, at enqueue time: the device
// entry points swap some of them for the caller's for the length of one enqueue. ----

// an opposite pair of paths along x (axis 0) or y (axis 1), not the final pass
static PairArgs pair_args(const fsgm_epi_plan* p, int f0, int axis = 0) {
    const size_t o = (size_t)f0, ckb = pair_ckpt_bytes(p->W, p->H, p->D, axis);
    PairArgs a{};
    a.C = p->dC + o * p->N; a.c_frame_stride = p->N;
    a.X = frame_at(p->dLh, o * p->N); a.x_frame_stride = p->N;
    a.ckpt = frame_at(axis ? p->dCkptV : p->dCkpt, o * ckb); a.ckpt_frame_stride = ckb;
    a.W = p->W; a.H = p->H; a.D = p->D; a.P1 = p->P1; a.P2 = p->P2;
    return a;
}

// a sweep of the block-sweep pipelines: a final one adds Y_h and writes the WTA records, the others write their Y only
static SweepArgs sweep_args(const fsgm_epi_plan* p, int f0, bool final = true) {
    const size_t o = (size_t)f0;
    SweepArgs a{};
    a.C = p->dC + o * p->N; a.c_frame_stride = p->N;
    a.X = p->dX + o * p->N; a.x_frame_stride = p->N;
    a.Lh = p->dLh + o * p->N; a.lh_frame_stride = p->N; a.lh_natural = p->form.x_fine;
    a.rec = p->dRec + o * p->NP; a.s0 = p->dS0 + o * p->NP;
    a.state_frame_stride = sweep_state_bytes(p->W, p->D);
    a.state_in = a.state_out = p->dState + 2 * o * a.state_frame_stride;
    a.W = p->W; a.H = p->H; a.D = p->D; a.P1 = p->P1; a.P2 = p->P2; a.y0 = 0; a.rows = 0;
    if (!final) { a.Lh = nullptr; a.lh_frame_stride = 0; a.lh_natural = 0; a.rec = nullptr; a.s0 = nullptr; }
    return a;
}

// the line kernels over `slots` path slots a frame, into L
static AggArgs agg_args(const fsgm_epi_plan* p, uint8_t* L, int slots) {
    AggArgs a;
    a.C = p->dC; a.L = L; a.c_frame_stride = p->N; a.l_frame_stride = slots * p->N; a.l_dir_stride = p->N;
    a.W = p->W; a.H = p->H; a.D = p->D; a.P1 = p->P1; a.P2 = p->P2;
    a.adaptive = p->adaptive; a.I1 = p->adaptive ? p->dI1 : nullptr; a.i_frame_stride = p->NP;
    return a;
}

static BandArgs band_args(const fsgm_epi_plan* p, int f0) {
    const size_t o = (size_t)f0;
    BandArgs a{};
    a.C = p->dC + o * p->N; a.c_frame_stride = p->N;
    a.Y = p->dX + o * p->N; a.y_frame_stride = p->N;
    a.yb_frame_stride = band_bits_u32s(p->W, p->H, p->D);
    a.Yb = frame_at(p->dBits, o * a.yb_frame_stride);
    a.edge_frame_stride = p->band_edge_maps * band_edge_uint4s(p->W, p->D, 8);
    a.edge = p->dBandEdge + o * a.edge_frame_stride;
    a.rec = p->dRec + o * p->NP; a.s0 = p->dS0 + o * p->NP; a.Sdbg = nullptr;
    a.W = p->W; a.H = p->H; a.D = p->D; a.P1 = p->P1; a.P2 = p->P2;
    a.chain = p->pipe == PIPE_BAND_CHAIN ? 1 : 0;
    a.frames = p->batch; a.nbands = (p->H + band_rows(p->D) - 1) / band_rows(p->D);
    a.group = p->batch;                                  // frames whose bands are dealt band-major: all (groups of 16-64 measured: no gain)
    a.ticket = p->dBandTicket; a.err = p->dBandErr;
    return a;
}

// vz_to_disp: the runs convert after the forward-backward check (prm.vz_to_disp && !prm.fb_check), the S tap in place
static WtaArgs wta_args(const fsgm_epi_plan* p, int f0, int vz_to_disp) {
    const size_t o = (size_t)f0 * p->NP;
    WtaArgs a{};
    a.off = frame_at(p->dOff, o); a.bestD = p->dBestD + o; a.minC = p->dMinC + o; a.vMax = p->vMax;
    a.W = p->W; a.H = p->H; a.D = p->D; a.ndirs = p->prm.paths;
    a.subpixel = p->prm.subpixel; a.vz_to_disp = vz_to_disp;
    a.minC2 = p->runner_up ? p->dMinC2 + o : nullptr;            // (on: the plan is on the line kernels, select_kernel)
    return a;
}

// the parallel sweeps' S = 8 (C + bias) - (Y_dn + Y_up + Y_h), or with the along-x lines 6 (C + bias) - (Y_dn + Y_up) + L_fwd + L_bwd
static SweepSumArgs sum_args(const fsgm_epi_plan* p, int f0) {
    const size_t o = (size_t)f0 * p->N;
    SweepSumArgs q{};
    q.C = p->dC + o; q.Xdn = frame_at(p->dX, o); q.Xup = frame_at(p->dXupAll, o); q.v_frame_stride = p->N;
    q.Lh = p->dLh + o; q.lh_frame_stride = p->N; q.lh_natural = p->form.x_fine;
    q.nC = 8; q.bias = p->P2 + p->P1; q.Sdbg = nullptr;
    if (p->form.x_lines) { q.Lh = nullptr; q.Lx = p->dLx + 2 * o; q.lx_frame_stride = 2 * p->N; q.nC = 6; }
    return q;
}

// ---- the pipelines: each one's aggregation and its S debug tap (fsgm_epi_plan_download_sum: frame f's S into dS) ----

// per-direction line kernels: the path volumes L, then a WTA kernel over them
static fsgm_status agg_lines(fsgm_epi_plan* p) {
    const int kind = p->pipe == PIPE_GENERIC ? AGG_GENERIC : p->pipe == PIPE_PACKED_WRAP ? AGG_PACKED_WRAP
                   : p->pipe == PIPE_PACKED_EXACT ? AGG_PACKED_EXACT : p->pipe == PIPE_GENERIC_EXACT ? AGG_GENERIC_EXACT : AGG_PACKED_NOWRAP;
    launch_aggregate(p->stream, agg_args(p, p->dL, p->prm.paths), p->prm.paths, p->batch, kind);
    return FSGM_OK;
}
static void tap_lines(fsgm_epi_plan* p, int f) {
    if (pipe_exact(p->pipe))                             // the volumes hold L - C: the frame's costs come back in
        return launch_sum_paths_exact(p->stream, p->dL + (size_t)f * p->N * p->prm.paths, p->dC + (size_t)f * p->N, p->dS, p->N, p->N,
                                      p->prm.paths);
    launch_sum_paths(p->stream, p->dL + (size_t)f * p->N * p->prm.paths, p->dS, p->N, p->N, p->prm.paths);
}

// 4 paths: the horizontal pair -> X_h on stream_h while the vertical pair's checkpoint pass runs
// here; then the vertical sum pass adds X_h + 4*C and does the WTA (7.5 B per voxel, S never in HBM)
static fsgm_status agg_pairs(fsgm_epi_plan* p) {
    FSGM_HIP(hipEventRecord(p->ev_fork, p->stream));
    FSGM_HIP(hipStreamWaitEvent(p->stream_h, p->ev_fork, 0));
    const PairArgs h = pair_args(p, 0);
    if (p->form.x_fine) launch_pair_x_fine(p->stream_h, h, p->batch);   // its chain is what this pipeline waits for
    else                launch_pair(p->stream_h, h, p->batch, 0, false);
    FSGM_HIP(hipEventRecord(p->ev_h, p->stream_h));
    PairArgs v = pair_args(p, 0, 1);
    v.X = nullptr; v.x_frame_stride = 0;
    v.Xother = p->dLh; v.xo_frame_stride = p->N; v.xo_natural = p->form.x_fine;
    v.rec = p->dRec; v.s0 = p->dS0; v.nC = 4;
    launch_pair(p->stream, v, p->batch, 1, true, 1);
    FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_h, 0));
    launch_pair(p->stream, v, p->batch, 1, true, 2);
    return FSGM_OK;
}
// materialise the vertical pair's X_v of that frame with a non-final sum pass into dXup (one frame of scratch: dX is a
// whole-batch buffer of other pipelines), then wta_sweep_kernel rebuilds S = X_v + X_h + 4C
static void tap_pairs(fsgm_epi_plan* p, int f) {
    PairArgs v = pair_args(p, f, 1);
    v.X = p->dXup;
    launch_pair(p->stream, v, 1, 1, false);
    SweepSumArgs q = sum_args(p, f);
    q.Xdn = p->dXup; q.Xup = nullptr; q.nC = 4; q.Sdbg = p->dS;
    launch_wta_sweep(p->stream, wta_args(p, f, p->prm.vz_to_disp), q, 1);
}

// One sweep launch (strips x frames workgroups) cannot fill 256 CUs, so the work is forked:
// the horizontal pair runs on stream_h, and the frames split into two lanes (one for a single frame),
// each sweeping down and then up (the final up sweep needs its lane's X_dn and the horizontal pair).
static fsgm_status agg_sweep(fsgm_epi_plan* p) {
    const int lanes = std::min(2, p->batch), first[3] = {0, (p->batch + 1) / 2, p->batch};   // lane l: frames [first[l], first[l + 1])
    const hipStream_t lane_stream[2] = {p->stream, p->stream_b};
    FSGM_HIP(hipEventRecord(p->ev_fork, p->stream));
    FSGM_HIP(hipStreamWaitEvent(p->stream_h, p->ev_fork, 0));
    if (lanes > 1) FSGM_HIP(hipStreamWaitEvent(p->stream_b, p->ev_fork, 0));
    // the two horizontal paths as one sum Y_h, lane by lane: a lane's final sweep waits for its own frames only
    for (int l = 0; l < lanes; l++) {
        launch_pair(p->stream_h, pair_args(p, first[l]), first[l + 1] - first[l], 0, false);
        FSGM_HIP(hipEventRecord(p->ev_hl[l], p->stream_h));
    }
    for (int l = 0; l < lanes; l++) {
        const SweepArgs w = sweep_args(p, first[l]);
        const int nf = first[l + 1] - first[l];
        launch_sweep(lane_stream[l], w, nf, 0);                  // pass-0 paths from above -> Y_dn
        FSGM_HIP(hipStreamWaitEvent(lane_stream[l], p->ev_hl[l], 0));
        launch_sweep(lane_stream[l], w, nf, 2);                  // pass-1 paths + everything else + WTA
    }
    if (lanes > 1) {
        FSGM_HIP(hipEventRecord(p->ev_b, p->stream_b));
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_b, 0));
    }
    return FSGM_OK;
}

// Parallel sweeps: three independent chains, the horizontal pair (stream_h), the down sweep (here), the up sweep (stream_b)
static fsgm_status agg_par_sweeps(fsgm_epi_plan* p) {
    FSGM_HIP(hipEventRecord(p->ev_fork, p->stream));
    FSGM_HIP(hipStreamWaitEvent(p->stream_h, p->ev_fork, 0));
    FSGM_HIP(hipStreamWaitEvent(p->stream_b, p->ev_fork, 0));
    // small batches wait for the pair's serial chain (3 x W steps): 8 costs a lane shorten it (Y_h then in natural d order)
    if (p->form.x_lines) {
        // few frames: the two along-x paths as line kernels (hand-written step, chains of W steps instead of the pair's 3 W;
        // L_fwd and L_bwd written out: 2 B per voxel more than Y_h, added up by the WTA kernel)
        launch_aggregate(p->stream_h, agg_args(p, p->dLx, 2), 2, p->batch, AGG_PACKED_NOWRAP);
    }
    else if (p->form.x_fine) launch_pair_x_fine(p->stream_h, pair_args(p, 0), p->batch);
    else                     launch_pair(p->stream_h, pair_args(p, 0), p->batch, 0, false);
    FSGM_HIP(hipEventRecord(p->ev_h, p->stream_h));
    const SweepArgs fin = sweep_args(p, 0);
    SweepArgs dn = sweep_args(p, 0, false), up = dn;
    up.X = p->dXupAll; up.state_in = up.state_out = p->dStateUp;
    const int tall = p->form.tall;                                // 8-wave workgroups: half the launches of a sweep
    if (p->pipe == PIPE_SWEEP_MID) {
        // the sweeps meet in the middle: rows [0, hm) of the frame belong to the down sweep's first half, rows [hm, H) to the
        // up sweep's (its rows [0, H - hm) of the mirrored frame); then each crosses the other's half as a final sweep
        const int hm = meet_row(p->H, p->D);
        int par_dn = 0, par_up = 0;
        launch_sweep_rows(p->stream, dn, p->batch, 0, tall, 0, hm, &par_dn);                 // -> Y_dn of rows [0, hm)
        FSGM_HIP(hipEventRecord(p->ev_c, p->stream));
        launch_sweep_rows(p->stream_b, up, p->batch, 1, tall, 0, p->H - hm, &par_up);         // -> Y_up of rows [hm, H)
        FSGM_HIP(hipEventRecord(p->ev_b, p->stream_b));
        SweepArgs dnf = fin, upf = fin;                                                     // what a final sweep reads: the other's Y
        dnf.X = p->dXupAll;
        upf.X = p->dX; upf.state_in = upf.state_out = p->dStateUp;
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_h, 0));
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_b, 0));
        launch_sweep_rows(p->stream, dnf, p->batch, 3, p->form.mid_tall, hm, p->H, &par_dn);       // rows [hm, H): + Y_up + Y_h, WTA
        FSGM_HIP(hipStreamWaitEvent(p->stream_b, p->ev_h, 0));
        FSGM_HIP(hipStreamWaitEvent(p->stream_b, p->ev_c, 0));
        launch_sweep_rows(p->stream_b, upf, p->batch, 2, p->form.mid_tall, p->H - hm, p->H, &par_up);  // rows [0, hm): + Y_dn + Y_h, WTA
        FSGM_HIP(hipEventRecord(p->ev_hl[0], p->stream_b));
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_hl[0], 0));
    } else {
        launch_sweep(p->stream, dn, p->batch, 0, tall);               // pass-0 paths from above -> Y_dn
        launch_sweep(p->stream_b, up, p->batch, 1, tall);             // pass-1 paths -> Y_up
        FSGM_HIP(hipEventRecord(p->ev_b, p->stream_b));
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_h, 0));
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->ev_b, 0));
    }
    return FSGM_OK;
}
// S never exists in HBM in sweep mode.  Debug tap: materialise X_up of that frame with a non-final up sweep into dXup
// (frame f's boundary states are idle now: scratch), then let wta_sweep_kernel rebuild S = X_dn + X_up + 6C + L_left + L_right.
static void tap_sweep(fsgm_epi_plan* p, int f) {
    SweepArgs w = sweep_args(p, f, false);
    w.X = p->dXup;
    launch_sweep(p->stream, w, 1, 1);
    if (p->pipe == PIPE_SWEEP_MID) {                             // the meeting sweeps leave Y_dn for the upper half of the rows only
        w.X = p->dX + (size_t)f * p->N;
        launch_sweep(p->stream, w, 1, 0);
    }
    SweepSumArgs q = sum_args(p, f);
    q.Xup = p->dXup; q.Sdbg = p->dS;
    launch_wta_sweep(p->stream, wta_args(p, f, p->prm.vz_to_disp), q, 1);
}

// all four paths of a raster pass in one sweep, one workgroup per frame: first pass -> Y (+ 9th bits), second pass + WTA
static fsgm_status agg_band(fsgm_epi_plan* p) {
    BandArgs b = band_args(p, 0);
    if (b.chain && p->band_edge_untagged) {              // words of the sequential form / the S tap could pass for tag 0: all ones is never a tag
        FSGM_HIP(hipMemsetAsync(p->dBandEdge, 0xFF, (size_t)p->batch * b.edge_frame_stride * sizeof(uint4), p->stream));
        p->band_edge_untagged = false;
    }
    if (!b.chain) p->band_edge_untagged = true;
    for (int mode = 0; mode <= 2; mode += 2) {
        if (b.chain) {                                   // the work counter restarts on the stream ahead of every launch; a fresh hand-off tag
            const uint32_t t = p->band_salt++ % 15u;     // 0..14: the all-ones pattern of the initial fill is never a valid tag
            b.tag = ((t & 1u) << 7) | ((t & 2u) << 14) | ((t & 4u) << 21) | ((t & 8u) << 28);
            FSGM_HIP(hipMemsetAsync(b.ticket, 0, sizeof(uint32_t), p->stream));
        }
        launch_band(p->stream, b, p->batch, p->prm.paths, mode);
    }
    return FSGM_OK;
}
// S never exists in HBM in band mode either.  Debug tap: the second pass of that frame again, in the sequential form (its
// first pass's Y is still in place), with the kernel's natural-order dump of S switched on.
static void tap_band(fsgm_epi_plan* p, int f) {
    BandArgs b = band_args(p, f);
    b.chain = 0; b.Sdbg = p->dS;                         // (frames, nbands, group, ticket, err: read by the chained form only)
    launch_band(p->stream, b, 1, p->prm.paths, 2);
    p->band_edge_untagged = true;
}

// (Replaying the fused-sweep stage -- ~100 launches on three streams -- as one HIP graph was measured on MI355X / ROCm 7.2, 32 frames,
// same box, alternating runs: 9 % SLOWER, 5.23 vs 4.79 ms per step; the runtime does not overlap the three captured branches as well
// as the three streams do.  Removed in round 3.)
static fsgm_status enqueue(fsgm_epi_plan* p, int stages) {
    fsgm_status st = prepare(p, stages);
    if (st != FSGM_OK) return st;
    if (stages & FSGM_STAGE_COST) {
        if ((st = ensure_vz(p)) != FSGM_OK) return st;
        enqueue_cost(p, 0, p->batch);
    }
    if (stages & FSGM_STAGE_AGGREGATE) {
        switch (p->pipe) {
            case PIPE_SWEEP: st = agg_sweep(p); break;
            case PIPE_SWEEP_PAR: case PIPE_SWEEP_MID: st = agg_par_sweeps(p); break;
            case PIPE_PAIRS: st = agg_pairs(p); break;
            case PIPE_BAND: case PIPE_BAND_CHAIN: st = agg_band(p); break;
            default: st = agg_lines(p); break;
        }
        if (st != FSGM_OK) return st;
    }
    if (stages & FSGM_STAGE_WTA) {
        WtaArgs a = wta_args(p, 0, p->prm.vz_to_disp && !p->prm.fb_check);
        if (p->pipe == PIPE_SWEEP_PAR) {                 // S = 8 (C + P2) - (Y_dn + Y_up + Y_h), argmin, parabola, vz -> disp
            launch_wta_sweep(p->stream, a, sum_args(p, 0), p->batch);
        } else if (!pipe_lines(p->pipe)) {               // the argmin happened inside the final sweep / pair pass
            launch_sweep_finish(p->stream, a, p->dRec, p->dS0, p->batch);
        } else {                                         // a WTA kernel over the path volumes
            a.L = p->dL; a.l_frame_stride = p->N * p->prm.paths; a.l_dir_stride = p->N;
            const WtaCostArgs x{pipe_exact(p->pipe) ? p->dC : nullptr, p->N};
            launch_wta(p->stream, a, p->batch, agg_line_split(p->D), x);
            if (p->view2) {                              // the second view's WTA over the same volumes (epi_view2.hip)
                View2Args v{};
                v.L = p->dL; v.l_frame_stride = a.l_frame_stride; v.l_dir_stride = a.l_dir_stride;
                v.C = x.C; v.c_frame_stride = x.c_frame_stride;
                v.disp2 = p->dDisp2v; v.minC2v = p->dMinCv2;
                v.W = p->W; v.H = p->H; v.D = p->D; v.ndirs = p->prm.paths; v.dir = p->v2_dir; v.d_min = p->d_min;
                v.subpixel = p->prm.subpixel; v.add = p->v2_add; v.marker = p->v2_marker;
                launch_view2(p->stream, v, p->batch);
            }
        }
    }
    if ((stages & FSGM_STAGE_WTA) && p->prm.fb_check) {
        // the check sees bestD before the vz conversion (order of calc_cost_sgm.cpp:584-594)
        FbArgs b;
        b.D1 = p->dBestD; b.pd0 = p->dPd0; b.nd = p->dNd; b.off = p->dOff;
        b.D2enc = p->dD2enc; b.D2 = p->dD2; b.conf = p->dConf;
        b.vMax = p->vMax; b.W = p->W; b.H = p->H; b.n = p->D + 1; b.thr = 2;      // :483 thr = 2
        b.linear = p->sampling != FSGM_SAMPLING_VZ; b.rect = p->direction; b.rect_shift = p->direction * p->d_min;
        launch_fb_check(p->stream, b, p->batch);
        if (p->prm.vz_to_disp) launch_vz_convert(p->stream, p->dBestD, p->dOff, p->W, p->H, p->D, p->vMax, p->batch);
    }
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_run(fsgm_epi_plan* p, int32_t stages) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE((stages & ~FSGM_STAGE_ALL) == 0 && stages != 0, "bad stage mask %d", stages);
    FSGM_HIP(hipSetDevice(p->prm.device));
    return enqueue(p, stages);
}

fsgm_status fsgm_epi_plan_set_agg_mode(fsgm_epi_plan* p, int32_t mode) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(mode >= 0 && mode <= 6, "agg mode must be 0 (auto), 1 (per-direction kernels), 2 (fused sweeps), 3 (parallel sweeps), 4 (band sweeps), 5 (chained band sweeps) or 6 (sweeps meeting in the middle)");
    if (p->adaptive && mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "agg mode %d on an adaptive-P2 plan: only the line kernels (modes 0 and 1) take a per-step P2", mode);
    if (p->runner_up && mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "agg mode %d on a runner-up plan: only the line kernels' WTA (modes 0 and 1) writes the runner-up cost", mode);
    if (p->exact && mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "agg mode %d on an exact plan: only the line kernels (modes 0 and 1) carry path costs above 255", mode);
    if (p->view2 && mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "agg mode %d on a second-view plan: only the line kernels (modes 0 and 1) keep the path volumes", mode);
    p->agg_mode = mode;
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_adaptive_p2(fsgm_epi_plan* p, int32_t on) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_adaptive_p2: on must be 0 or 1 (got %d)", on);
    if (on && p->agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "adaptive P2 on a plan forced to agg mode %d: only the line kernels (modes 0 and 1) take a per-step P2",
                    p->agg_mode);
    p->adaptive = on;
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_runner_up(fsgm_epi_plan* p, int32_t on) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_runner_up: on must be 0 or 1 (got %d)", on);
    if (on && p->agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "runner-up cost on a plan forced to agg mode %d: only the line kernels' WTA (modes 0 and 1) writes it",
                    p->agg_mode);
    if (on && p->exact)
        return fail(FSGM_ERR_UNSUPPORTED, "runner-up cost on an exact plan: the exact WTA writes no second minimum");
    if (on && !p->dMinC2) {                                      // all ones until a WTA has run: FSGM_NO_RUNNER_UP
        const size_t bytes = (size_t)p->batch * p->NP * 4;
        uint32_t* m = nullptr;
        FSGM_HIP(hipSetDevice(p->prm.device));
        FSGM_HIP(hipMalloc((void**)&m, bytes));
        const hipError_t e = hipMemsetAsync(m, 0xFF, bytes, p->stream);
        if (e != hipSuccess) { (void)hipFree(m); return hip_status(e, "fsgm_epi_plan_set_runner_up"); }
        p->dMinC2 = m;
    }
    p->runner_up = on;
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_exact(fsgm_epi_plan* p, int32_t on) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_exact: on must be 0 or 1 (got %d)", on);
    if (on && p->agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "exact path arithmetic on a plan forced to agg mode %d: only the line kernels (modes 0 and 1) carry path costs above 255",
                    p->agg_mode);
    if (on && p->runner_up)
        return fail(FSGM_ERR_UNSUPPORTED, "exact path arithmetic on a runner-up plan: the exact WTA writes no second minimum");
    FSGM_REQUIRE(!on || (p->P1 >= 0 && p->P1 <= 255 && p->P2 >= 0 && p->P2 <= 255),
                 "fsgm_epi_plan_set_exact: an exact plan takes P1 and P2 in 0..255 (the plan holds %d, %d)", p->P1, p->P2);
    p->exact = on;
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_view2(fsgm_epi_plan* p, int32_t on, int32_t direction) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_view2: on must be 0 or 1 (got %d)", on);
    if (!on) { p->view2 = 0; select_kernel(p); return FSGM_OK; }
    FSGM_REQUIRE(direction == -1 || direction == 1, "fsgm_epi_plan_set_view2: direction must be -1 or +1 (got %d)", direction);
    if (p->sampling == FSGM_SAMPLING_LINEAR || (p->sampling == FSGM_SAMPLING_VZ && p->prm.vz_to_disp))
        return fail(FSGM_ERR_UNSUPPORTED, "second view on a plan with the vz sampling or per-pixel direction maps: its candidates share no line");
    FSGM_REQUIRE(p->sampling != FSGM_SAMPLING_RECTIFIED || direction == p->direction,
                 "fsgm_epi_plan_set_view2: a rectified plan's second view has the plan's direction %d (got %d)", p->direction, direction);
    if (p->agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "second view on a plan forced to agg mode %d: only the line kernels (modes 0 and 1) keep the path volumes",
                    p->agg_mode);
    if (!p->dDisp2v) {                                           // all ones until a WTA has run: FSGM_NO_VIEW2
        const size_t bytes = (size_t)p->batch * p->NP * 4;
        FSGM_HIP(hipSetDevice(p->prm.device));
        LazySet ls;
        uint32_t* d = ls.alloc(p->dDisp2v, bytes);
        uint32_t* m = ls.alloc(p->dMinCv2, bytes);
        if (ls.err == hipSuccess) ls.err = hipMemsetAsync(d, 0xFF, bytes, p->stream);
        if (ls.err == hipSuccess) ls.err = hipMemsetAsync(m, 0xFF, bytes, p->stream);
        if (ls.err != hipSuccess) return lazy_fail(ls, "fsgm_epi_plan_set_view2");
        ls.commit();
    }
    p->view2 = 1; p->v2_dir = direction;
    select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_download_view2(fsgm_epi_plan* p, int32_t f, uint32_t* disp2, uint32_t* minC_v2) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(f >= 0 && f < p->batch, "frame %d out of range (batch %d)", f, p->batch);
    FSGM_REQUIRE(p->view2, "fsgm_epi_plan_download_view2: the plan's second-view switch is off (fsgm_epi_plan_set_view2)");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    if (disp2) FSGM_HIP(hipMemcpy(disp2, p->dDisp2v + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    if (minC_v2) FSGM_HIP(hipMemcpy(minC_v2, p->dMinCv2 + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_view2_launch_lds(int32_t dMax, uint64_t* bytes) {
    FSGM_REQUIRE(bytes, "fsgm_view2_launch_lds: null argument");
    FSGM_REQUIRE(dMax >= 1 && dMax <= FSGM_GENERIC_MAX_D, "fsgm_view2_launch_lds: dMax must be 1..%d (got %d)", FSGM_GENERIC_MAX_D, dMax);
    *bytes = view2_lds_bytes(dMax);
    return FSGM_OK;
}

int32_t fsgm_view2_tile(int32_t dMax) { return dMax >= 1 && dMax <= FSGM_GENERIC_MAX_D ? view2_tile(dMax) : 0; }

fsgm_status fsgm_epi_plan_set_d_min(fsgm_epi_plan* p, int32_t d_min) {
    FSGM_REQUIRE(p, "null plan");
    if (p->sampling != FSGM_SAMPLING_RECTIFIED)
        return fail(FSGM_ERR_UNSUPPORTED, "fsgm_epi_plan_set_d_min: only a rectified plan has a disparity range to move (the caller of the others owns the maps)");
    FSGM_REQUIRE(d_min >= -FSGM_D_MIN_LIMIT && d_min <= FSGM_D_MIN_LIMIT, "fsgm_epi_plan_set_d_min: |d_min| must be <= %d (got %d)", FSGM_D_MIN_LIMIT, d_min);
    p->d_min = d_min;                                            // read by the next cost stage and forward-backward check
    return FSGM_OK;
}

fsgm_epi_options fsgm_epi_options_default(void) {
    fsgm_epi_options o;
    memset(&o, 0, sizeof(o));
    return o;
}

// the options of an *_opts entry point (null: the defaults), checked
static fsgm_status read_options(const char* who, const fsgm_epi_options* opt, fsgm_epi_options* o) {
    *o = opt ? *opt : fsgm_epi_options_default();
    FSGM_REQUIRE(o->adaptive_p2 == 0 || o->adaptive_p2 == 1, "%s: adaptive_p2 must be 0 or 1 (got %d)", who, o->adaptive_p2);
    for (int r : o->reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_epi_options must be zero", who);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_sync(fsgm_epi_plan* p) {
    FSGM_REQUIRE(p, "null plan");
    return frame_ready(p, 0, 2);                                 // (frame 0: every plan has it)
}

fsgm_status fsgm_epi_plan_download(fsgm_epi_plan* p, int32_t f, uint32_t* bestD, uint32_t* minC) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    if (bestD) FSGM_HIP(hipMemcpy(bestD, p->dBestD + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    if (minC) FSGM_HIP(hipMemcpy(minC, p->dMinC + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_download_fb(fsgm_epi_plan* p, int32_t f, uint8_t* conf, uint32_t* bestD2) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    FSGM_REQUIRE(p->prm.fb_check, "the plan was created without fb_check");
    if (conf) FSGM_HIP(hipMemcpy(conf, p->dConf + f * p->NP, p->NP, hipMemcpyDeviceToHost));
    if (bestD2) FSGM_HIP(hipMemcpy(bestD2, p->dD2 + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_download_runner_up(fsgm_epi_plan* p, int32_t f, uint32_t* minC2) {
    FSGM_REQUIRE(p && minC2, "fsgm_epi_plan_download_runner_up: null argument");
    FSGM_REQUIRE(f >= 0 && f < p->batch, "frame %d out of range (batch %d)", f, p->batch);
    FSGM_REQUIRE(p->runner_up, "fsgm_epi_plan_download_runner_up: the plan's runner-up switch is off (fsgm_epi_plan_set_runner_up)");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    FSGM_HIP(hipMemcpy(minC2, p->dMinC2 + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_download_cost(fsgm_epi_plan* p, int32_t f, uint8_t* C) {
    FSGM_REQUIRE(p && C, "fsgm_epi_plan_download_cost: null argument");
    { fsgm_status fs = frame_ready(p, f, 1); if (fs != FSGM_OK) return fs; }
    FSGM_HIP(hipMemcpy(C, p->dC + f * p->N, p->N, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_download_census(fsgm_epi_plan* p, int32_t f, uint32_t* cen1, uint32_t* cen2) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 1); if (fs != FSGM_OK) return fs; }
    FSGM_REQUIRE(p->dCen1, "fsgm_epi_plan_download_census: the cost stage has not run on this plan");
    if (cen1) FSGM_HIP(hipMemcpy(cen1, p->dCen1 + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    if (cen2) FSGM_HIP(hipMemcpy(cen2, p->dCen2 + f * p->NP, p->NP * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

// the S tap's own buffers (one frame each), created on first use
static fsgm_status ensure_tap_buffers(fsgm_epi_plan* p) {
    if (!p->dS) FSGM_HIP(hipMalloc((void**)&p->dS, p->N * 4));
    if (!p->dXup && (pipe_sweep(p->pipe) || p->pipe == PIPE_PAIRS)) FSGM_HIP(hipMalloc((void**)&p->dXup, p->N));
    return FSGM_OK;
}
// frame f's S into dS on the plan's stream, by the selected pipeline's tap
static void tap_sum(fsgm_epi_plan* p, int f) {
    switch (p->pipe) {
        case PIPE_SWEEP: case PIPE_SWEEP_PAR: case PIPE_SWEEP_MID: tap_sweep(p, f); break;
        case PIPE_PAIRS: tap_pairs(p, f); break;
        case PIPE_BAND: case PIPE_BAND_CHAIN: tap_band(p, f); break;
        default: tap_lines(p, f); break;
    }
}

fsgm_status fsgm_epi_plan_download_sum(fsgm_epi_plan* p, int32_t f, uint32_t* S) {
    FSGM_REQUIRE(p && S, "fsgm_epi_plan_download_sum: null argument");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    // the line kernels sum the frame's path volumes; the fused pipelines never hold S in HBM and rebuild it (tap_*)
    { fsgm_status es = ensure_agg_buffers(p); if (es != FSGM_OK) return es; }
    { fsgm_status es = ensure_tap_buffers(p); if (es != FSGM_OK) return es; }
    tap_sum(p, f);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipStreamSynchronize(p->stream));
    FSGM_HIP(hipMemcpy(S, p->dS, p->N * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_time(fsgm_epi_plan* p, int32_t stages, int32_t warmup, int32_t iters, float* ms_avg) {
    FSGM_REQUIRE(p && ms_avg, "fsgm_epi_plan_time: null argument");
    FSGM_REQUIRE(iters >= 1 && warmup >= 0, "fsgm_epi_plan_time: iters must be >= 1");
    FSGM_REQUIRE((stages & ~FSGM_STAGE_ALL) == 0 && stages != 0, "bad stage mask %d", stages);
    FSGM_HIP(hipSetDevice(p->prm.device));
    const fsgm_status st = time_enqueues(p->stream, p->ev0, p->ev1, warmup, iters, [&] { return enqueue(p, stages); }, ms_avg);
    if (st != FSGM_OK) return st;
    return check_handoff(p);                                     // a timed run that gave up on a hand-off is not a measurement
}

void* fsgm_epi_plan_stream(fsgm_epi_plan* p) { return p ? (void*)p->stream : nullptr; }

const char* fsgm_epi_plan_kernel_name(fsgm_epi_plan* p) {
    if (!p) return "";
    return kPipelineName[p->pipe];
}

const char* fsgm_epi_auto_pipeline(int32_t width, int32_t height, int32_t dMax, int32_t batch, int32_t paths, int32_t P1, int32_t P2,
                                   int32_t cmax, int32_t cus) {
    if (width <= 0 || height <= 0 || dMax <= 0 || batch <= 0 || (paths != 4 && paths != 8) || cus <= 0) return "";
    return kPipelineName[choose_pipeline(width, height, dMax, batch, paths, P1, P2, cmax, 0, cus)];
}

const char* fsgm_epi_auto_pipeline_opts(int32_t width, int32_t height, int32_t dMax, int32_t batch, int32_t paths, int32_t P1, int32_t P2,
                                        int32_t cmax, int32_t cus, const fsgm_epi_options* opt) {
    if (width <= 0 || height <= 0 || dMax <= 0 || batch <= 0 || (paths != 4 && paths != 8) || cus <= 0) return "";
    return kPipelineName[choose_pipeline(width, height, dMax, batch, paths, P1, P2, cmax, 0, cus, opt && opt->adaptive_p2)];
}

// the launchers' own selector (select_cost_kernels, epi_cost.hip) for a shape a plan of this sampling would accept
fsgm_status fsgm_epi_cost_kernels(int32_t W, int32_t H, int32_t dMax, int32_t sampling, char* buf, size_t buflen) {
    FSGM_REQUIRE(buf && buflen > 0, "fsgm_epi_cost_kernels: null or empty buffer");
    buf[0] = 0;
    { const fsgm_status as = epi_plan_args(W, H, dMax, 1, fsgm_epi_params_default(), sampling, -1); if (as != FSGM_OK) return as; }
    const bool rect = sampling == FSGM_SAMPLING_RECTIFIED;
    const char* name = cost_kernels_name(select_cost_kernels(W, H, dMax, rect), rect);
    FSGM_REQUIRE(strlen(name) < buflen, "fsgm_epi_cost_kernels: buffer of %zu bytes too small for \"%s\"", buflen, name);
    memcpy(buf, name, strlen(name) + 1);
    return FSGM_OK;
}

// The achievable HBM rate of this device, measured the way the aggregation kernels move bytes: a grid-stride
// copy kernel, 16 B per lane per access (launch_copy16, epi_kernels.hip), device memory to device memory, read + written
// bytes counted.  mode 0: that kernel; mode 1: hipMemcpyAsync D2D (the runtime's blit kernel), for comparison.
fsgm_status fsgm_measure_copy_bandwidth2(int32_t device, size_t bytes, int32_t iters, int32_t mode, double* gbps) {
    FSGM_REQUIRE(gbps && bytes >= 4096 && iters > 0, "fsgm_measure_copy_bandwidth: bad argument");
    FSGM_REQUIRE(mode == 0 || mode == 1, "fsgm_measure_copy_bandwidth: mode must be 0 (copy kernel) or 1 (hipMemcpyAsync)");
    FSGM_HIP(hipSetDevice(device));
    bytes &= ~(size_t)4095;
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0, e1;
    FSGM_HIP(hipMalloc(&a, bytes));
    if (hipMalloc(&b, bytes) != hipSuccess) { (void)hipFree(a); return fail(FSGM_ERR_NOMEM, "copy probe: out of memory"); }
    (void)hipMemset(a, 1, bytes);
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto once = [&]() {
        if (mode == 0) launch_copy16(0, b, a, bytes);
        else (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, 0);
    };
    once();
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < iters; i++) once();
    (void)hipEventRecord(e1, 0);
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    if (e != hipSuccess) return fail(FSGM_ERR_HIP, "copy probe: %s", hipGetErrorString(e));
    *gbps = 2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9;
    return FSGM_OK;
}

fsgm_status fsgm_measure_copy_bandwidth(int32_t device, size_t bytes, int32_t iters, double* gbps) {
    return fsgm_measure_copy_bandwidth2(device, bytes, iters, 0, gbps);
}

// ---------------------------------------------------------------------------------------------
// host-pointer entry points (the MEX boundary).  Plans are cached per shape for the lifetime of
// the process so repeated MEX calls do not re-allocate HBM (SURVEY 8b "ownership").
// ---------------------------------------------------------------------------------------------
// cached plans per device (the cap bounds the HBM held by stale shapes; a plan recorded into a graph is held beside them)
static PlanCache<fsgm_epi_plan> g_epi(4, fsgm_epi_plan_destroy, [](const fsgm_epi_plan* p) { return p->pinned; });

// The cached plan of this shape for an entry point: `lk` holds its device's lock for the length of the call, the device is current.
// (a plan serves one sampling mode and, rectified, one direction: the modes share no cached state)
static fsgm_status cached_plan(std::unique_lock<std::mutex>& lk, fsgm_epi_plan** out, int W, int H, int D, int batch,
                               const fsgm_epi_params& pr, int sampling = FSGM_SAMPLING_VZ, int direction = 0, int adaptive = 0,
                               int agg_mode = 0, int runner_up = 0, int exact = 0, bool must_exist = false,
                               int view2_dir = 0) {
    FSGM_DEVICE_SLOT(pr.device);
    lk = std::unique_lock<std::mutex>(g_epi.mu(pr.device));
    fsgm_epi_plan* p = g_epi.find(pr.device, [&](const fsgm_epi_plan* q) {
        return q->W == W && q->H == H && q->D == D && q->batch == batch && q->prm.paths == pr.paths &&
               q->prm.fb_check == pr.fb_check && q->prm.vz_to_disp == pr.vz_to_disp && q->sampling == sampling &&
               q->direction == direction && q->adaptive == adaptive &&   // (adaptive and non-adaptive callers never share a plan)
               q->agg_mode == agg_mode &&                                // (nor do forced modes: only the sgm batch forms ask for one)
               q->runner_up == runner_up &&                              // (nor a runner-up caller and a plain one: the plain call keeps its pipeline)
               q->exact == exact &&                                      // (nor an exact caller and a plain one)
               q->view2 == (view2_dir != 0) && (!view2_dir || q->v2_dir == view2_dir);   // (nor a second-view caller and a plain one)
    });
    if (p) p->prm = pr;
    else if (must_exist)                                         // (a captured call: creating a plan allocates, copies and waits)
        return fail(FSGM_ERR_UNSUPPORTED, "the stream is being captured into a graph and no call of this shape and these switches has run yet: "
                                          "run it once outside the capture");
    else {
        fsgm_status st = fsgm_epi_plan_create_sampling(&p, W, H, D, batch, &pr, sampling, direction);
        if (st == FSGM_OK && adaptive && (st = fsgm_epi_plan_set_adaptive_p2(p, 1)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        else if (st == FSGM_OK && agg_mode && (st = fsgm_epi_plan_set_agg_mode(p, agg_mode)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        else if (st == FSGM_OK && runner_up && (st = fsgm_epi_plan_set_runner_up(p, 1)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        else if (st == FSGM_OK && exact && (st = fsgm_epi_plan_set_exact(p, 1)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        else if (st == FSGM_OK && view2_dir && (st = fsgm_epi_plan_set_view2(p, 1, view2_dir)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        if (st != FSGM_OK) return st;
        g_epi.insert(pr.device, p);
    }
    *out = p;
    FSGM_HIP(hipSetDevice(pr.device));
    return FSGM_OK;
}

void fsgm_pyd_shutdown_internal(void);
void fsgm_pyramid_shutdown_internal(void);
void fsgm_post_shutdown_internal(void);
void fsgm_ng_shutdown_internal(void);
void fsgm_ng_pyramid_shutdown_internal(void);
void fsgm_flow_pp_shutdown_internal(void);
void fsgm_stereo_pp_shutdown_internal(void);
void fsgm_sgm2d_shutdown_internal(void);

void fsgm_shutdown(void) {
    fsgm_sgm2d_shutdown_internal();
    fsgm_stereo_pp_shutdown_internal();
    fsgm_flow_pp_shutdown_internal();
    fsgm_ng_pyramid_shutdown_internal();
    fsgm_ng_shutdown_internal();
    fsgm_post_shutdown_internal();
    fsgm_pyramid_shutdown_internal();
    fsgm_pyd_shutdown_internal();
    g_epi.clear();
}

// calc_cost_sgm on host pointers in either build of the reference: vz-index sampling, or linear (offset and vMax unused)
static fsgm_status epi_batch_host(int sampling, int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                  const fsgm_epi_options* opt) {
    FSGM_REQUIRE(n >= 1 && in && out, "fsgm_calc_cost_sgm: null argument");
    fsgm_epi_options o;
    { const fsgm_status os = read_options("fsgm_calc_cost_sgm", opt, &o); if (os != FSGM_OK) return os; }
    fsgm_epi_params pr = prm ? *prm : fsgm_epi_params_default();
    const bool linear = sampling == FSGM_SAMPLING_LINEAR;
    if (linear) pr.vz_to_disp = 0;
    for (int i = 0; i < n; i++) {
        FSGM_REQUIRE(in[i].I1 && in[i].I2 && in[i].pixelPosD0 && in[i].normDir && (in[i].offset || linear),
                     "fsgm_calc_cost_sgm: frame %d has a null input", i);
        FSGM_REQUIRE(out[i].bestD && out[i].minC, "fsgm_calc_cost_sgm: frame %d has a null output", i);
        FSGM_REQUIRE(in[i].width == in[0].width && in[i].height == in[0].height && in[i].dMax == in[0].dMax &&
                     in[i].P1 == in[0].P1 && in[i].P2 == in[0].P2 && (linear || in[i].vMax == in[0].vMax),
                     "fsgm_calc_cost_sgm: frames of one batch must share shape and parameters (frame %d differs)", i);
    }
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, in[0].width, in[0].height, in[0].dMax, n, pr, sampling, 0, o.adaptive_p2);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, in[0].P1, in[0].P2, linear ? p->vMax : in[0].vMax)) != FSGM_OK) return st;
    if ((st = ensure_cost_buffers(p)) != FSGM_OK) return st;
    p->have_img.assign(n, 1);                                    // every frame's pair goes up below, ahead of the kernels
    // One call = one stream-ordered sequence with a single host wait: every frame's inputs go up asynchronously on the
    // plan's stream (hipMemcpyAsync from the caller's pageable memory runs at the pinned rate here, ~50 GB/s, so there is
    // no staging copy: tools/ubench/h2d_rates.hip), the batched kernels follow, the results come down at the end.
    // Measured alternatives that lost (A/B on one box): uploads on a second stream with each frame's cost stage started
    // as the frame arrives -- the per-frame launches cost more than the overlap saves (1.29 vs 1.20 ms for one
    // 1242x375x128 frame, 9.2 vs 7.9 ms for eight); a pinned staging ring (an extra host copy at 25-34 GB/s).
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    const size_t NP = p->NP;
    for (int i = 0; i < n; i++)
        if ((st = upload_async(p, i, in[i].I1, in[i].I2, in[i].pixelPosD0, in[i].normDir, in[i].offset)) != FSGM_OK) return st;
    if ((st = enqueue(p, FSGM_STAGE_ALL)) != FSGM_OK) return st;
    bool taps = false;
    for (int i = 0; i < n; i++) {
        FSGM_HIP(hipMemcpyAsync(out[i].bestD, p->dBestD + i * NP, NP * 4, hipMemcpyDeviceToHost, p->stream));
        FSGM_HIP(hipMemcpyAsync(out[i].minC, p->dMinC + i * NP, NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (pr.fb_check && out[i].conf) FSGM_HIP(hipMemcpyAsync(out[i].conf, p->dConf + i * NP, NP, hipMemcpyDeviceToHost, p->stream));
        if (pr.fb_check && out[i].bestD2) FSGM_HIP(hipMemcpyAsync(out[i].bestD2, p->dD2 + i * NP, NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (out[i].C) FSGM_HIP(hipMemcpyAsync(out[i].C, p->dC + (size_t)i * p->N, p->N, hipMemcpyDeviceToHost, p->stream));
        taps = taps || out[i].S;
    }
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    if ((st = check_handoff(p)) != FSGM_OK) return st;
    if (taps)
        for (int i = 0; i < n; i++)
            if (out[i].S && (st = fsgm_epi_plan_download_sum(p, i, out[i].S)) != FSGM_OK) return st;
    return FSGM_OK;
}

fsgm_status fsgm_calc_cost_sgm_batch_host_opts(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                               const fsgm_epi_options* opt) {
    return epi_batch_host(FSGM_SAMPLING_VZ, n, in, out, prm, opt);
}
fsgm_status fsgm_calc_cost_sgm_host_opts(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                         const fsgm_epi_options* opt) {
    return epi_batch_host(FSGM_SAMPLING_VZ, 1, in, out, prm, opt);
}
fsgm_status fsgm_calc_cost_sgm_linear_batch_host_opts(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out,
                                                      const fsgm_epi_params* prm, const fsgm_epi_options* opt) {
    return epi_batch_host(FSGM_SAMPLING_LINEAR, n, in, out, prm, opt);
}
fsgm_status fsgm_calc_cost_sgm_linear_host_opts(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                                const fsgm_epi_options* opt) {
    return epi_batch_host(FSGM_SAMPLING_LINEAR, 1, in, out, prm, opt);
}

// the entry points without options: the same calls with every option off
fsgm_status fsgm_calc_cost_sgm_batch_host(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm) {
    return fsgm_calc_cost_sgm_batch_host_opts(n, in, out, prm, nullptr);
}

fsgm_status fsgm_calc_cost_sgm_host(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm) {
    return fsgm_calc_cost_sgm_batch_host_opts(1, in, out, prm, nullptr);
}

fsgm_status fsgm_calc_cost_sgm_linear_batch_host(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm) {
    return fsgm_calc_cost_sgm_linear_batch_host_opts(n, in, out, prm, nullptr);
}

fsgm_status fsgm_calc_cost_sgm_linear_host(const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm) {
    return fsgm_calc_cost_sgm_linear_batch_host_opts(1, in, out, prm, nullptr);
}

// ---- rectified stereo on host pointers: n contiguous frames, images up, everything else as calc_cost_sgm ----
fsgm_stereo_params fsgm_stereo_params_default(void) {
    fsgm_stereo_params p;
    p.paths = 4; p.subpixel = 1; p.fb_check = 0; p.direction = -1; p.device = 0;
    return p;
}

// the pipeline of this thread's last rectified-stereo one-shot call (fsgm_stereo_sgm_last_kernel), as fsgm_sgm_last_kernel's
static thread_local const char* g_stereo_kernel = "";

static fsgm_status stereo_args(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                               const fsgm_stereo_params* prm, const uint32_t* disp, const uint32_t* minC, fsgm_stereo_params* sp,
                               fsgm_epi_params* pr) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(I1 && I2 && disp && minC, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1 && dMax >= 1, "%s: width/height/dMax must be >= 1 (got %d x %d x %d)", who, W, H, dMax);
    *sp = prm ? *prm : fsgm_stereo_params_default();
    FSGM_REQUIRE(sp->direction == -1 || sp->direction == 1, "%s: direction must be -1 (match at x - d) or +1 (x + d), got %d", who, sp->direction);
    *pr = fsgm_epi_params_default();
    pr->paths = sp->paths; pr->subpixel = sp->subpixel; pr->fb_check = sp->fb_check; pr->device = sp->device; pr->vz_to_disp = 0;
    return FSGM_OK;
}

fsgm_status fsgm_stereo_sgm_host(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                 int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp, uint32_t* minC, uint8_t* conf,
                                 uint32_t* disp2) {
    return fsgm_stereo_sgm_host_opts(n, I1, I2, W, H, dMax, P1, P2, prm, nullptr, disp, minC, conf, disp2);
}

// The cached rectified plan is shared by every d_min (the key does not hold it): each stereo entry point sets the plan's shift
// under the plan's lock before it queues anything, the older ones to 0.  ranged: the _range forms, whose disp / disp2 leave as
// int32 true disparities.
// the one-shot entries' left-right check buffer [batch][NP]
static fsgm_status ensure_view2_conf(fsgm_epi_plan* p) {
    if (!p->dConfV2) FSGM_HIP(hipMalloc((void**)&p->dConfV2, (size_t)p->batch * p->NP));
    return FSGM_OK;
}
// the view-2 forms' own arguments (include/fsgm.h, "Second view"): disp2 required, minC_v2 and conf may be NULL
struct StereoView2 {
    int max_diff;
    uint32_t *disp2, *minC_v2;
    uint8_t* conf;
};
static fsgm_status stereo_view2_args(const char* who, const fsgm_stereo_params& sp, const StereoView2& v) {
    FSGM_REQUIRE(v.disp2, "%s: null disp2", who);
    FSGM_REQUIRE(v.max_diff >= 0, "%s: max_diff must be >= 0 (got %d)", who, v.max_diff);
    FSGM_REQUIRE(!sp.fb_check, "%s: fb_check = 1 is the forward-backward check of fsgm_stereo_sgm_host (the other door): not together with the second view", who);
    return FSGM_OK;
}
// the plan's second view as int32 true disparities for the length of one enqueue
struct View2Format {
    fsgm_epi_plan* p;
    View2Format(fsgm_epi_plan* q, int d_min) : p(q) { p->v2_add = (uint32_t)(256 * d_min); p->v2_marker = 0x80000000u; }
    ~View2Format() { p->v2_add = 0; p->v2_marker = 0xFFFFFFFFu; }
};
// the left-right check on a stereo call's outputs, int32 true disparities both
static void enqueue_stereo_view2_check(fsgm_epi_plan* p, int dir, int max_diff, int n, const uint32_t* disp, const uint32_t* disp2, uint8_t* conf) {
    View2CheckArgs k{};
    k.disp = disp; k.disp2 = disp2; k.conf = conf; k.W = p->W; k.H = p->H; k.dir = dir; k.max_diff = max_diff;
    k.add1 = k.add2 = 0; k.marker2 = 0x80000000u;
    if (!p->prm.subpixel) { k.pre1 = k.add1 = 256 * p->d_min; k.shift1 = 8; }   // (disp = 256 * d_min + the whole index, as the _range forms return it)
    launch_view2_check(p->stream, k, n);
}

static fsgm_status stereo_host(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                               int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                               bool ranged, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2, uint32_t* minC2 = nullptr,
                               const StereoView2* v2 = nullptr) {
    fsgm_stereo_params sp;
    fsgm_epi_params pr;
    fsgm_epi_options o;
    fsgm_status st = stereo_args(who, n, I1, I2, W, H, dMax, prm, disp, minC, &sp, &pr);
    if (st != FSGM_OK) return st;
    if ((st = read_options(who, opt, &o)) != FSGM_OK) return st;
    FSGM_REQUIRE(d_min >= -FSGM_D_MIN_LIMIT && d_min <= FSGM_D_MIN_LIMIT, "%s: |d_min| must be <= %d (got %d)", who, FSGM_D_MIN_LIMIT, d_min);
    if (v2 && (st = stereo_view2_args(who, sp, *v2)) != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    if ((st = cached_plan(lk, &p, W, H, dMax, n, pr, FSGM_SAMPLING_RECTIFIED, sp.direction, o.adaptive_p2, 0, minC2 != nullptr, 0, false,
                          v2 ? sp.direction : 0)) != FSGM_OK) return st;
    p->d_min = d_min;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    if ((st = ensure_cost_buffers(p)) != FSGM_OK) return st;
    if (v2 && v2->conf && (st = ensure_view2_conf(p)) != FSGM_OK) return st;
    p->have_img.assign(n, 1);                                    // the pairs go up below, ahead of the kernels
    const size_t np = (size_t)n * p->NP;
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    FSGM_HIP(hipMemcpyAsync(p->dI1, I1, np, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dI2, I2, np, hipMemcpyHostToDevice, p->stream));
    if (v2) { View2Format fmt(p, d_min); st = enqueue(p, FSGM_STAGE_ALL); }
    else st = enqueue(p, FSGM_STAGE_ALL);
    if (st != FSGM_OK) return st;
    g_stereo_kernel = kPipelineName[p->pipe];
    if (ranged) {
        launch_stereo_range(p->stream, p->dBestD, pr.fb_check ? p->dD2 : nullptr, np, d_min);
        FSGM_HIP(hipGetLastError());
    }
    FSGM_HIP(hipMemcpyAsync(disp, p->dBestD, np * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (minC2) FSGM_HIP(hipMemcpyAsync(minC2, p->dMinC2, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (pr.fb_check && conf) FSGM_HIP(hipMemcpyAsync(conf, p->dConf, np, hipMemcpyDeviceToHost, p->stream));
    if (pr.fb_check && disp2) FSGM_HIP(hipMemcpyAsync(disp2, p->dD2, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (v2) {                                                    // (ranged: dBestD holds int32 true disparities by now)
        FSGM_HIP(hipMemcpyAsync(v2->disp2, p->dDisp2v, np * 4, hipMemcpyDeviceToHost, p->stream));
        if (v2->minC_v2) FSGM_HIP(hipMemcpyAsync(v2->minC_v2, p->dMinCv2, np * 4, hipMemcpyDeviceToHost, p->stream));
        if (v2->conf) {
            enqueue_stereo_view2_check(p, sp.direction, v2->max_diff, n, p->dBestD, p->dDisp2v, p->dConfV2);
            FSGM_HIP(hipGetLastError());
            FSGM_HIP(hipMemcpyAsync(v2->conf, p->dConfV2, np, hipMemcpyDeviceToHost, p->stream));
        }
    }
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return check_handoff(p);
}

fsgm_status fsgm_stereo_sgm_host_opts(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, uint32_t* disp,
                                      uint32_t* minC, uint8_t* conf, uint32_t* disp2) {
    return stereo_host("fsgm_stereo_sgm_host", n, I1, I2, W, H, dMax, P1, P2, prm, opt, 0, false, disp, minC, conf, disp2);
}

fsgm_status fsgm_stereo_sgm_host_range(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t* disp, uint32_t* minC, uint8_t* conf, int32_t* disp2) {
    return stereo_host("fsgm_stereo_sgm_host_range", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                       (uint32_t*)disp2);
}

const char* fsgm_stereo_sgm_last_kernel(void) { return g_stereo_kernel; }

// the same through a cached plan with the runner-up switch on (never the plan of the call above: cached_plan's key)
fsgm_status fsgm_stereo_sgm_host_ru(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                    int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                    int32_t* disp, uint32_t* minC, uint32_t* minC2, uint8_t* conf, int32_t* disp2) {
    FSGM_REQUIRE(minC2, "fsgm_stereo_sgm_host_ru: null minC2");
    return stereo_host("fsgm_stereo_sgm_host_ru", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                       (uint32_t*)disp2, minC2);
}

// the second view from the same aggregated volume and the left-right check against it (include/fsgm.h, "Second view")
fsgm_status fsgm_stereo_sgm_view2_host(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf) {
    const StereoView2 v{max_diff, (uint32_t*)disp2, minC_v2, conf};
    return stereo_host("fsgm_stereo_sgm_view2_host", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, nullptr,
                       nullptr, minC2, &v);
}

// sgm(C, P1, P2): sgm.m's call shape on the MEX's aggregation + WTA (MEX semantics: include/fsgm.h)
fsgm_status fsgm_sgm_host(const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2, int32_t paths,
                          uint32_t* bestD, uint32_t* minC, uint32_t* S, int32_t device) {
    FSGM_REQUIRE(C && bestD && minC, "fsgm_sgm: null argument");
    fsgm_epi_params pr = fsgm_epi_params_default();
    pr.paths = paths; pr.device = device; pr.vz_to_disp = 0; pr.subpixel = 1;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, W, H, D, 1, pr);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_upload_cost(p, 0, C)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_run(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_download(p, 0, bestD, minC)) != FSGM_OK) return st;
    if (S && (st = fsgm_epi_plan_download_sum(p, 0, S)) != FSGM_OK) return st;
    return FSGM_OK;
}

}  // extern "C"

// ---- sgm(C, P1, P2) on batches of caller-supplied volumes (capi_sgm.hip has checked the call) ----
namespace fsgm {

static thread_local const char* g_sgm_kernel = "";

// the cached plan of a checked call: its batch, mode, adaptive, runner-up and exact switches are part of the key
static fsgm_status sgm_plan(std::unique_lock<std::mutex>& lk, fsgm_epi_plan** p, const SgmCall& c) {
    fsgm_epi_params pr = fsgm_epi_params_default();
    pr.paths = c.prm.paths; pr.subpixel = c.prm.subpixel; pr.device = c.prm.device; pr.vz_to_disp = 0; pr.fb_check = 0;
    return cached_plan(lk, p, c.W, c.H, c.D, c.n, pr, FSGM_SAMPLING_VZ, 0, c.prm.adaptive_p2, c.prm.agg_mode, c.minC2 != nullptr, c.exact,
                       c.captured != 0, c.view2);
}

// the check of the sgm(C) view-2 forms on the plan's own outputs: index units, both shifted by the call's d_min
static void enqueue_sgm_view2_check(fsgm_epi_plan* p, const SgmCall& c, const uint32_t* bestD, const uint32_t* disp2, uint8_t* conf) {
    View2CheckArgs k{};
    k.disp = bestD; k.disp2 = disp2; k.conf = conf; k.W = p->W; k.H = p->H; k.dir = c.view2; k.max_diff = c.max_diff;
    k.add1 = k.add2 = 256 * c.d_min; k.marker2 = 0xFFFFFFFFu;
    k.shift1 = c.prm.subpixel ? 0 : 8;                           // (without sub-pixel bestD is the whole index, disp2 always index * 256)
    launch_view2_check(p->stream, k, c.n);
}

static fsgm_status ensure_ingest_flag(fsgm_epi_plan* p) {
    if (p->dIngestFlag) return FSGM_OK;
    FSGM_HIP(hipMalloc((void**)&p->dIngestFlag, sizeof(uint32_t)));
    FSGM_HIP(hipMemsetAsync(p->dIngestFlag, 0, sizeof(uint32_t), p->stream));
    return FSGM_OK;
}

fsgm_status sgm_run_host(const SgmCall& c, const int* cmax) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = sgm_plan(lk, &p, c);
    if (st != FSGM_OK) return st;
    const size_t NP = p->NP, nv = (size_t)c.n * p->N;
    for (int f = 0; f < c.n; f++) p->cmax[f] = cmax[f];
    if ((st = fsgm_epi_plan_set_penalties(p, c.P1, c.P2, p->vMax)) != FSGM_OK) return st;    // (selects the kernels for cmax)
    if (c.guide)                                                 // the aggregation reads I1 only: the guide stands for both images
        for (int f = 0; f < c.n; f++)
            if ((st = fsgm_epi_plan_upload_images(p, f, c.guide + f * NP, c.guide + f * NP)) != FSGM_OK) return st;
    if ((st = prepare(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    const bool dhw = c.prm.layout == FSGM_COST_LAYOUT_DHW;       // staged as it came, transposed on the device
    if (dhw && c.fmt.dtype < 0 && !p->dIngest) FSGM_HIP(hipMalloc((void**)&p->dIngest, nv));
    if (c.fmt.dtype >= 0 && (st = ensure_ingest_flag(p)) != FSGM_OK) return st;
    if (c.view2) p->d_min = c.d_min;                             // (read by the second view's kernel only: the plan has no cost stage to shift)
    if (c.conf && (st = ensure_view2_conf(p)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    if (c.fmt.dtype >= 0) {
        // a float volume: staged frame by frame, quantised by the kernel the device form runs; the flag is read before any output is written
        const fsgm_status fs = stage_float_volumes(p->stream, c.C, c.fmt, c.n, p->N, p->dIngestFlag, "fsgm_sgm_float_batch_host",
            [&](const void* d, int f) { launch_sgm_ingest_float(p->stream, d, c.fmt, p->dC + (size_t)f * p->N, 1, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag); });
        if (fs != FSGM_OK) return fs;
    } else {
        FSGM_HIP(hipMemcpyAsync(dhw ? p->dIngest : p->dC, c.C, nv, hipMemcpyHostToDevice, p->stream));
        if (dhw) launch_sgm_ingest(p->stream, p->dIngest, p->dC, c.n, c.W, c.H, c.D, FSGM_COST_LAYOUT_DHW, 255, nullptr);
    }
    if ((st = enqueue(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    g_sgm_kernel = kPipelineName[p->pipe];
    FSGM_HIP(hipMemcpyAsync(c.bestD, p->dBestD, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(c.minC, p->dMinC, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    if (c.minC2) FSGM_HIP(hipMemcpyAsync(c.minC2, p->dMinC2, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    if (c.view2) {
        FSGM_HIP(hipMemcpyAsync(c.disp2, p->dDisp2v, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (c.minC_v2) FSGM_HIP(hipMemcpyAsync(c.minC_v2, p->dMinCv2, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (c.conf) {
            enqueue_sgm_view2_check(p, c, p->dBestD, p->dDisp2v, p->dConfV2);
            FSGM_HIP(hipGetLastError());
            FSGM_HIP(hipMemcpyAsync(c.conf, p->dConfV2, (size_t)c.n * NP, hipMemcpyDeviceToHost, p->stream));
        }
    }
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    if ((st = check_handoff(p)) != FSGM_OK) return st;
    for (int f = 0; c.S && f < c.n; f++)
        if ((st = fsgm_epi_plan_download_sum(p, f, c.S + (size_t)f * p->N)) != FSGM_OK) return st;
    return FSGM_OK;
}

fsgm_status sgm_run_device(const SgmCall& c, hipStream_t cs, int32_t* status) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = sgm_plan(lk, &p, c);
    if (st != FSGM_OK) return st;
    if (c.captured) {
        // Under a capture nothing may be allocated or waited for: everything the call below would create must exist (an earlier
        // call of the host form, or one without S or without a guide, leaves some of it out).  Refused before anything is queued.
        const bool warm = p->dL && p->dIngestFlag && p->join.in && p->join.out && (!c.S || p->dS) && (!c.guide || (p->dI1 && p->dI2));
        if (!warm)
            return fail(FSGM_ERR_UNSUPPORTED, "fsgm_sgm_device_exact: the stream is being captured into a graph and the cached plan lacks buffers "
                                              "this call needs: run the same call once outside the capture");
        p->pinned = true;                                        // the graph names the plan's buffers, stream and events from here on
    }
    // What a warm call must not do happens here, before the join with the caller's stream.  The device cannot be asked for the
    // true maximum without a wait: the declared bound selects the kernels, the ingest kernel saturates at it.
    p->cmax.assign(c.n, c.prm.cost_bound);
    if ((st = fsgm_epi_plan_set_penalties(p, c.P1, c.P2, p->vMax)) != FSGM_OK) return st;
    if (c.guide) {
        if ((st = ensure_image_buffers(p)) != FSGM_OK) return st;
        p->have_img.assign(c.n, 1);                              // the guide goes into dI1 below, ahead of the kernels
    }
    if ((st = prepare(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    if ((st = ensure_ingest_flag(p)) != FSGM_OK) return st;
    if (c.S && (st = ensure_tap_buffers(p)) != FSGM_OK) return st;
    if (c.view2) p->d_min = c.d_min;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        if (c.fmt.dtype >= 0) launch_sgm_ingest_float(p->stream, c.C, c.fmt, p->dC, c.n, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        else launch_sgm_ingest(p->stream, c.C, p->dC, c.n, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        if (c.guide) FSGM_HIP(hipMemcpyAsync(p->dI1, c.guide, (size_t)c.n * p->NP, hipMemcpyDeviceToDevice, p->stream));
        Bind<uint32_t> bd(p->dBestD, c.bestD), mc(p->dMinC, c.minC), m2(p->dMinC2, c.minC2);
        Bind<uint32_t> d2(p->dDisp2v, c.disp2), mv(p->dMinCv2, c.minC_v2);   // (the view-2 forms: written where they lie)
        const fsgm_status es = enqueue(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA);
        if (es != FSGM_OK) return es;
        g_sgm_kernel = kPipelineName[p->pipe];
        if (c.view2 && c.conf) enqueue_sgm_view2_check(p, c, c.bestD, c.disp2, c.conf);
        for (int f = 0; c.S && f < c.n; f++) {                   // S never exists for a batch: frame by frame through the tap's buffer
            tap_sum(p, f);
            FSGM_HIP(hipMemcpyAsync(c.S + (size_t)f * p->N, p->dS, p->N * 4, hipMemcpyDeviceToDevice, p->stream));
        }
        launch_device_status(p->stream, p->dBandErr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

}  // namespace fsgm

extern "C" {

const char* fsgm_sgm_last_kernel(void) { return g_sgm_kernel; }

fsgm_status fsgm_epi_plan_ingest_cost_device(fsgm_epi_plan* p, int32_t n, const uint8_t* C, int32_t layout, int32_t cost_bound,
                                             void* stream, int32_t* status) {
    const char* who = "fsgm_epi_plan_ingest_cost_device";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    FSGM_REQUIRE(n == p->batch, "%s: n_frames %d differs from the plan's batch %d", who, n, p->batch);
    FSGM_REQUIRE(layout == FSGM_COST_LAYOUT_HWD || layout == FSGM_COST_LAYOUT_DHW,
                 "%s: layout must be FSGM_COST_LAYOUT_HWD (0) or FSGM_COST_LAYOUT_DHW (1), got %d", who, layout);
    FSGM_REQUIRE(cost_bound >= 1 && cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, cost_bound);
    const hipStream_t cs = (hipStream_t)stream;
    fsgm_status st;
    if ((st = device_check_args(who, p->prm.device, cs, {{C, (size_t)n * p->N, 1, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(p)) != FSGM_OK) return st;
    p->cmax.assign(n, cost_bound);
    select_kernel(p);
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm_ingest(p->stream, C, p->dC, n, p->W, p->H, p->D, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

fsgm_status fsgm_epi_plan_ingest_float_dptr(fsgm_epi_plan* p, int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t layout,
                                            int32_t cost_bound, void* stream, int32_t* status) {
    const char* who = "fsgm_epi_plan_ingest_float_dptr";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    CostFormat cf;
    fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(n == p->batch, "%s: n_frames %d differs from the plan's batch %d", who, n, p->batch);
    FSGM_REQUIRE(layout == FSGM_COST_LAYOUT_HWD || layout == FSGM_COST_LAYOUT_DHW,
                 "%s: layout must be FSGM_COST_LAYOUT_HWD (0) or FSGM_COST_LAYOUT_DHW (1), got %d", who, layout);
    FSGM_REQUIRE(cost_bound >= 1 && cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, cost_bound);
    const hipStream_t cs = (hipStream_t)stream;
    const size_t es = cost_elem_size(cf.dtype);
    if ((st = device_check_args(who, p->prm.device, cs, {{C, (size_t)n * p->N * es, es, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(p)) != FSGM_OK) return st;
    p->cmax.assign(n, cost_bound);
    select_kernel(p);
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm_ingest_float(p->stream, C, cf, p->dC, n, p->W, p->H, p->D, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

// census() of common.cpp:3-27 alone (the one function of the path that the reference's own sources pin here)
fsgm_status fsgm_census_host(const uint8_t* img, int32_t W, int32_t H, uint32_t* cen, int32_t device) {
    FSGM_REQUIRE(img && cen, "fsgm_census: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    fsgm_epi_params pr = fsgm_epi_params_default();
    pr.device = device;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, W, H, 16, 1, pr);       // any dMax: only the image / census buffers are used
    if (st != FSGM_OK) return st;
    if ((st = ensure_cost_buffers(p)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);
    FSGM_HIP(hipMemcpyAsync(p->dI1, img, p->NP, hipMemcpyHostToDevice, p->stream));
    launch_census(p->stream, p->dI1, p->dCen1, W, H, 1);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(cen, p->dCen1, p->NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

// ---- the dense half of the epipolar driver (dense part only) ----
static EpiGeomArgs geom_args(const fsgm_epi_geometry* g, int W, int H, double* Pd0, double* nd, double* off, double* rflow) {
    EpiGeomArgs a;
    for (int i = 0; i < 9; i++) { a.F[i] = g->F[i]; a.Hm[i] = g->H[i]; }
    a.ex = g->epipole[0]; a.ey = g->epipole[1]; a.direction = g->direction != 0;
    a.Pd0 = Pd0; a.nd = nd; a.off = off; a.rflow = rflow; a.W = W; a.H = H;
    return a;
}

// The epipolar drivers' buffers (RGB staging: host forms with RGB planes); test.m's frame body (pp) also has the
// post-processing chain's scratch plan and D1, and its host form flow2.
static fsgm_status ensure_driver_buffers(fsgm_epi_plan* p, int channels, bool pp = false, bool host = false) {
    { fsgm_status cs = ensure_cost_buffers(p); if (cs != FSGM_OK) return cs; }
    const size_t np = (size_t)p->batch * p->NP;
    if (!p->dRflow) FSGM_HIP(hipMalloc((void**)&p->dRflow, np * 16));
    if (!p->dFlow) FSGM_HIP(hipMalloc((void**)&p->dFlow, np * 24));
    if (channels == 3 && !p->dRgb) FSGM_HIP(hipMalloc((void**)&p->dRgb, p->NP * 3 * 2));
    if (pp && !p->post) {
        fsgm_status st = post_plan_create_batch(&p->post, p->W, p->H, p->batch, p->prm.device, false);
        if (st != FSGM_OK) return st;
    }
    if (pp && !p->dD1) FSGM_HIP(hipMalloc((void**)&p->dD1, np * 8));
    if (pp && host && !p->dFlow2) FSGM_HIP(hipMalloc((void**)&p->dFlow2, np * 24));
    return FSGM_OK;
}

fsgm_status fsgm_epipolar_maps_host(const fsgm_epi_geometry* g, int32_t W, int32_t H, double* Pd0, double* normDirect,
                                    double* Offset, double* Rflow, int32_t device) {
    FSGM_REQUIRE(g && Pd0 && normDirect && Offset && Rflow, "fsgm_epipolar_maps: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    fsgm_epi_params pr = fsgm_epi_params_default();
    pr.device = device;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, W, H, 16, 1, pr);       // any dMax: only the map buffers are used
    if (st != FSGM_OK) return st;
    if ((st = ensure_driver_buffers(p, 1)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);
    launch_epi_maps(p->stream, geom_args(g, W, H, p->dPd0, p->dNd, p->dOff, p->dRflow));
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(Pd0, p->dPd0, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(normDirect, p->dNd, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(Offset, p->dOff, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(Rflow, p->dRflow, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

// ---------------------------------------------------------------------------------------------
// device-pointer entry points (include/fsgm.h): the caller's HBM arrays stand in for the plan's image, map and result buffers
// for the length of one enqueue; the plan's stream is joined with the caller's at both ends.
// ---------------------------------------------------------------------------------------------
static fsgm_status epi_device_args(const char* who, int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, bool linear) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(in && out, "%s: null argument", who);
    FSGM_REQUIRE(in->I1 && in->I2 && in->pixelPosD0 && in->normDir && (in->offset || linear), "%s: null input", who);
    FSGM_REQUIRE(out->bestD && out->minC, "%s: null output", who);
    FSGM_REQUIRE(in->width >= 1 && in->height >= 1 && in->dMax >= 1, "%s: width/height/dMax must be >= 1 (got %d x %d x %d)", who,
                 in->width, in->height, in->dMax);
    if (out->C || out->S) return fail(FSGM_ERR_UNSUPPORTED, "%s: the debug taps C / S are not offered on device pointers", who);
    return FSGM_OK;
}

// What a warm call must not do -- allocate, upload a table, synchronise -- happens here on a plan's first call, before the
// join with the caller's stream (device_call).
static fsgm_status epi_device_prepare(fsgm_epi_plan* p, int P1, int P2, double vMax) {
    fsgm_status st;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, vMax)) != FSGM_OK) return st;
    if ((st = ensure_cost_buffers(p)) != FSGM_OK) return st;
    if ((st = ensure_vz(p)) != FSGM_OK) return st;
    p->have_img.assign(p->batch, 1);                             // the caller's images stand in for the plan's for this enqueue
    return prepare(p, FSGM_STAGE_ALL);
}

// a batch on device pointers through the caller's plan p, or (p null) through the cached plan for prm
static fsgm_status epi_run_device(const char* who, fsgm_epi_plan* p, const fsgm_epi_params* prm, int32_t n, const fsgm_epi_in* in,
                                  const fsgm_epi_out* out, void* stream, int32_t* status, int sampling = FSGM_SAMPLING_VZ,
                                  const fsgm_epi_options* opt = nullptr) {
    const bool linear = (p ? p->sampling : sampling) == FSGM_SAMPLING_LINEAR;
    fsgm_status st = epi_device_args(who, n, in, out, linear);
    if (st != FSGM_OK) return st;
    fsgm_epi_params pr = prm ? *prm : fsgm_epi_params_default();   // (the cached plan's key; a caller's plan has its own)
    fsgm_epi_options o{};
    if (p) {
        FSGM_REQUIRE(p->sampling != FSGM_SAMPLING_RECTIFIED, "%s: a rectified plan runs through fsgm_stereo_sgm_device", who);
        FSGM_REQUIRE(n == p->batch, "%s: n_frames %d differs from the plan's batch %d", who, n, p->batch);
        FSGM_REQUIRE(in->width == p->W && in->height == p->H && in->dMax == p->D, "%s: shape %d x %d x %d differs from the plan's %d x %d x %d",
                     who, in->width, in->height, in->dMax, p->W, p->H, p->D);
        pr = p->prm;
    } else {
        if (linear) pr.vz_to_disp = 0;
        if ((st = read_options(who, opt, &o)) != FSGM_OK) return st;
        FSGM_DEVICE_SLOT(pr.device);
        if ((st = epi_plan_args(in->width, in->height, in->dMax, n, pr, sampling, 0)) != FSGM_OK) return st;
    }
    const hipStream_t cs = (hipStream_t)stream;
    const size_t np = (size_t)n * in->width * in->height;
    const bool fb = pr.fb_check != 0;
    if ((st = device_check_args(who, pr.device, cs, {{in->I1, np, 1, true, "I1"},
                                                     {in->I2, np, 1, true, "I2"},
                                                     {in->pixelPosD0, np * 16, 8, true, "pixelPosD0"},
                                                     {in->normDir, np * 16, 8, true, "normDir"},
                                                     {linear ? nullptr : in->offset, np * 8, 8, !linear, "offset"},
                                                     {out->bestD, np * 4, 4, true, "bestD"},
                                                     {out->minC, np * 4, 4, true, "minC"},
                                                     {fb ? out->conf : nullptr, np, 1, false, "conf"},
                                                     {fb ? out->bestD2 : nullptr, np * 4, 4, false, "bestD2"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    if (!p && (st = cached_plan(lk, &p, in->width, in->height, in->dMax, n, pr, sampling, 0, o.adaptive_p2)) != FSGM_OK) return st;
    if ((st = epi_device_prepare(p, in->P1, in->P2, linear ? p->vMax : in->vMax)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, const_cast<uint8_t*>(in->I1)), i2(p->dI2, const_cast<uint8_t*>(in->I2));
        Bind<double> pd0(p->dPd0, const_cast<double*>(in->pixelPosD0)), nd(p->dNd, const_cast<double*>(in->normDir));
        Bind<double> off(p->dOff, linear ? nullptr : const_cast<double*>(in->offset));   // (linear: the plan's own 1.0 map)
        Bind<uint32_t> bd(p->dBestD, out->bestD), mc(p->dMinC, out->minC), d2(p->dD2, fb ? out->bestD2 : nullptr);
        Bind<uint8_t> conf(p->dConf, fb ? out->conf : nullptr);
        const fsgm_status es = enqueue(p, FSGM_STAGE_ALL);
        if (es == FSGM_OK) launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return es;
    });
}

fsgm_status fsgm_epi_plan_run_device(fsgm_epi_plan* p, int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, void* stream,
                                     int32_t* status) {
    FSGM_REQUIRE(p, "fsgm_epi_plan_run_device: null plan");
    return epi_run_device("fsgm_epi_plan_run_device", p, nullptr, n, in, out, stream, status);
}

fsgm_status fsgm_calc_cost_sgm_device_opts(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                           const fsgm_epi_options* opt, void* stream, int32_t* status) {
    return epi_run_device("fsgm_calc_cost_sgm_device", nullptr, prm, n, in, out, stream, status, FSGM_SAMPLING_VZ, opt);
}

fsgm_status fsgm_calc_cost_sgm_linear_device_opts(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                                  const fsgm_epi_options* opt, void* stream, int32_t* status) {
    return epi_run_device("fsgm_calc_cost_sgm_linear_device", nullptr, prm, n, in, out, stream, status, FSGM_SAMPLING_LINEAR, opt);
}

fsgm_status fsgm_calc_cost_sgm_device(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                      void* stream, int32_t* status) {
    return fsgm_calc_cost_sgm_device_opts(n, in, out, prm, nullptr, stream, status);
}

fsgm_status fsgm_calc_cost_sgm_linear_device(int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                             void* stream, int32_t* status) {
    return fsgm_calc_cost_sgm_linear_device_opts(n, in, out, prm, nullptr, stream, status);
}

fsgm_status fsgm_stereo_sgm_device(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                   int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp, uint32_t* minC, uint8_t* conf,
                                   uint32_t* disp2, void* stream, int32_t* status) {
    return fsgm_stereo_sgm_device_opts(n, I1, I2, W, H, dMax, P1, P2, prm, nullptr, disp, minC, conf, disp2, stream, status);
}

// (the shift and the cached plan: as stereo_host)
static fsgm_status stereo_device(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                                 int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                 bool ranged, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2, void* stream,
                                 int32_t* status, uint32_t* minC2 = nullptr, const StereoView2* v2 = nullptr) {
    fsgm_stereo_params sp;
    fsgm_epi_params pr;
    fsgm_epi_options o;
    fsgm_status st = stereo_args(who, n, I1, I2, W, H, dMax, prm, disp, minC, &sp, &pr);
    if (st != FSGM_OK) return st;
    if ((st = read_options(who, opt, &o)) != FSGM_OK) return st;
    FSGM_REQUIRE(d_min >= -FSGM_D_MIN_LIMIT && d_min <= FSGM_D_MIN_LIMIT, "%s: |d_min| must be <= %d (got %d)", who, FSGM_D_MIN_LIMIT, d_min);
    if (v2 && (st = stereo_view2_args(who, sp, *v2)) != FSGM_OK) return st;
    const size_t np = (size_t)n * (size_t)W * (size_t)H;
    const bool fb = pr.fb_check != 0;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, pr.device, cs, {{I1, np, 1, true, "I1"},
                                                     {I2, np, 1, true, "I2"},
                                                     {disp, np * 4, 4, true, "disp"},
                                                     {minC, np * 4, 4, true, "minC"},
                                                     {minC2, np * 4, 4, false, "minC2"},
                                                     {fb ? conf : nullptr, np, 1, false, "conf"},
                                                     {fb ? disp2 : nullptr, np * 4, 4, false, "disp2"},
                                                     {v2 ? v2->disp2 : nullptr, np * 4, 4, v2 != nullptr, "disp2"},
                                                     // (the label carries the type for the reason given at fsgm_sgm_view2_dptr's table, capi_sgm.hip)
                                                     {v2 ? v2->minC_v2 : nullptr, np * 4, 4, false, "minC_v2 (u32)"},
                                                     {v2 ? v2->conf : nullptr, np, 1, false, "conf"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    if ((st = cached_plan(lk, &p, W, H, dMax, n, pr, FSGM_SAMPLING_RECTIFIED, sp.direction, o.adaptive_p2, 0, minC2 != nullptr, 0, false,
                          v2 ? sp.direction : 0)) != FSGM_OK) return st;
    p->d_min = d_min;
    if ((st = epi_device_prepare(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, const_cast<uint8_t*>(I1)), i2(p->dI2, const_cast<uint8_t*>(I2));
        Bind<uint32_t> bd(p->dBestD, disp), mc(p->dMinC, minC), d2(p->dD2, fb ? disp2 : nullptr), m2(p->dMinC2, minC2);
        Bind<uint8_t> cf(p->dConf, fb ? conf : nullptr);
        Bind<uint32_t> v2d(p->dDisp2v, v2 ? v2->disp2 : nullptr), v2m(p->dMinCv2, v2 ? v2->minC_v2 : nullptr);
        fsgm_status es;
        if (v2) { View2Format fmt(p, d_min); es = enqueue(p, FSGM_STAGE_ALL); }
        else es = enqueue(p, FSGM_STAGE_ALL);
        if (es != FSGM_OK) return es;
        g_stereo_kernel = kPipelineName[p->pipe];
        if (ranged) launch_stereo_range(p->stream, disp, fb ? disp2 : nullptr, np, d_min);
        if (v2 && v2->conf) enqueue_stereo_view2_check(p, sp.direction, v2->max_diff, n, disp, v2->disp2, v2->conf);
        launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return FSGM_OK;
    });
}

fsgm_status fsgm_stereo_sgm_device_opts(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                        int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, uint32_t* disp,
                                        uint32_t* minC, uint8_t* conf, uint32_t* disp2, void* stream, int32_t* status) {
    return stereo_device("fsgm_stereo_sgm_device", n, I1, I2, W, H, dMax, P1, P2, prm, opt, 0, false, disp, minC, conf, disp2, stream, status);
}

fsgm_status fsgm_stereo_sgm_device_range(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                         int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                         int32_t* disp, uint32_t* minC, uint8_t* conf, int32_t* disp2, void* stream, int32_t* status) {
    return stereo_device("fsgm_stereo_sgm_device_range", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                         (uint32_t*)disp2, stream, status);
}

// fsgm_stereo_sgm_host_ru on device pointers: minC2 is written where it lies, by the WTA itself
fsgm_status fsgm_stereo_sgm_device_ru(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                      int32_t* disp, uint32_t* minC, uint32_t* minC2, uint8_t* conf, int32_t* disp2, void* stream,
                                      int32_t* status) {
    FSGM_REQUIRE(minC2, "fsgm_stereo_sgm_device_ru: null minC2");
    return stereo_device("fsgm_stereo_sgm_device_ru", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                         (uint32_t*)disp2, stream, status, minC2);
}

// fsgm_stereo_sgm_view2_host on device pointers: disp2, minC_v2 and conf are written where they lie
fsgm_status fsgm_stereo_sgm_view2_dptr(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf, void* stream, int32_t* status) {
    const StereoView2 v{max_diff, (uint32_t*)disp2, minC_v2, conf};
    return stereo_device("fsgm_stereo_sgm_view2_dptr", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, nullptr,
                         nullptr, stream, status, minC2, &v);
}

// ---------------------------------------------------------------------------------------------
// The epipolar drivers: epipolar_sgm_of (the matcher, then the flow) and test.m's frame body (pp; :32-54), the geometry given:
// the matcher in vz-index mode, D1 = bestD/256, flow, the post-processing chain and flow2, all on the plan's stream
// ---------------------------------------------------------------------------------------------
// the arguments of both forms of test.m's frame body (pp: flow2 required) and of fsgm_epipolar_sgm_of_device
static fsgm_status driver_args(const char* who, bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H,
                               int32_t channels, const fsgm_epi_geometry* g, int32_t dMax, const fsgm_epi_params* prm, const double* flow,
                               const double* flow2, fsgm_epi_params* pr) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(I0 && I1 && g && flow && (flow2 || !pp), "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1 && dMax >= 1, "%s: width/height/dMax must be >= 1 (got %d x %d x %d)", who, W, H, dMax);
    FSGM_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 (gray) or 3 (RGB planes), got %d", who, channels);
    *pr = prm ? *prm : fsgm_epi_params_default();
    if (!pp) {
        FSGM_REQUIRE(pr->vz_to_disp && !pr->fb_check, "%s: the flow needs disparities (vz_to_disp = 1, fb_check = 0)", who);
    } else {
        FSGM_REQUIRE(!pr->fb_check, "%s: fb_check must be 0 (the chain does its own forward-backward check)", who);
        if ((double)n * W * H >= 2147483648.0)
            return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, (double)n * W * H);
    }
    if (pp) pr->vz_to_disp = 0;                                                          // the chain works on vz indices
    return FSGM_OK;
}

// images in dI1 / dI2 and the maps in dPd0 / dNd / dOff / dRflow: the matcher (epipolar_sgm_of.m:45, test.m:36), then each
// frame's flow (epipolar_sgm_of.m:46-51) or (pp) test.m's flow (:38-42) and flow2 (:45-54); D1 [batch][H][W]
static fsgm_status enqueue_flow(fsgm_epi_plan* p, bool pp, int dMax, double vMax, double* flow, double* flow2, double* D1) {
    fsgm_status st = enqueue(p, FSGM_STAGE_ALL);
    if (st != FSGM_OK) return st;
    const int W = p->W, H = p->H, nf = p->batch;
    const size_t NP = p->NP;
    if (!pp) {
        for (int f = 0; f < nf; f++)
            launch_epi_flow(p->stream, p->dBestD + f * NP, p->dNd + f * 2 * NP, p->dRflow + f * 2 * NP, flow + f * 3 * NP, W, H);
    } else {
        const double n = (double)dMax + 1.0;                                             // test.m:6
        const PostScratch s = post_plan_scratch(p->post);
        launch_vz_from_bestd(p->stream, p->dBestD, D1, (size_t)nf * NP);
        post_enqueue_batch(p->stream, s, nf, W, H, D1, p->dPd0, p->dNd, p->dOff, vMax, n, (double)dMax, s.B, s.D2, nullptr, nullptr);
        launch_epi_pp_flow(p->stream, D1, s.B, p->dOff, p->dNd, p->dRflow, flow, flow2, W, H, nf, vMax, n);
    }
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

// Host forms: on the plan's stream the n image pairs as gray (:35-38; RGB planes through one staging pair, reused in stream
// order) and each frame's coordinate maps (:24), the matcher (:45) and the flow (:46-51), the results down.
static fsgm_status host_drive(bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                              const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params& pr, double* flow,
                              double* flow2, double* D1, uint32_t* minC) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, W, H, dMax, n, pr);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, 6, 64, vMax)) != FSGM_OK) return st;       // epipolar_sgm_of.m:19, test.m:36
    if ((st = ensure_driver_buffers(p, channels, pp, true)) != FSGM_OK) return st;
    const size_t NP = p->NP, np = (size_t)n * NP;
    StreamGuard guard(p->stream);
    if (channels == 1) {
        FSGM_HIP(hipMemcpyAsync(p->dI1, I0, np, hipMemcpyHostToDevice, p->stream));
        FSGM_HIP(hipMemcpyAsync(p->dI2, I1, np, hipMemcpyHostToDevice, p->stream));
    }
    for (int f = 0; f < n; f++) {
        if (channels == 3) {
            FSGM_HIP(hipMemcpyAsync(p->dRgb, I0 + f * 3 * NP, 3 * NP, hipMemcpyHostToDevice, p->stream));
            FSGM_HIP(hipMemcpyAsync(p->dRgb + 3 * NP, I1 + f * 3 * NP, 3 * NP, hipMemcpyHostToDevice, p->stream));
            launch_pyr_gray(p->stream, p->dRgb, p->dI1 + f * NP, W, H);
            launch_pyr_gray(p->stream, p->dRgb + 3 * NP, p->dI2 + f * NP, W, H);
        }
        launch_epi_maps(p->stream, geom_args(&g[f], W, H, p->dPd0 + f * 2 * NP, p->dNd + f * 2 * NP, p->dOff + f * NP, p->dRflow + f * 2 * NP));
    }
    if ((st = enqueue_flow(p, pp, dMax, vMax, p->dFlow, p->dFlow2, p->dD1)) != FSGM_OK) return st;
    FSGM_HIP(hipMemcpyAsync(flow, p->dFlow, np * 24, hipMemcpyDeviceToHost, p->stream));
    if (flow2) FSGM_HIP(hipMemcpyAsync(flow2, p->dFlow2, np * 24, hipMemcpyDeviceToHost, p->stream));
    if (D1) FSGM_HIP(hipMemcpyAsync(D1, p->dD1, np * 8, hipMemcpyDeviceToHost, p->stream));
    if (minC) FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, np * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return check_handoff(p);
}

fsgm_status fsgm_epipolar_sgm_of_host(const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                      const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                      double* flow, uint32_t* minC) {
    FSGM_REQUIRE(I0 && I1 && g && flow, "fsgm_epipolar_sgm_of: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    FSGM_REQUIRE(channels == 1 || channels == 3, "channels must be 1 (gray) or 3 (RGB planes), got %d", channels);
    fsgm_epi_params pr = prm ? *prm : fsgm_epi_params_default();
    FSGM_REQUIRE(pr.vz_to_disp && !pr.fb_check, "fsgm_epipolar_sgm_of: the flow needs disparities (vz_to_disp = 1, fb_check = 0)");
    return host_drive(false, 1, I0, I1, W, H, channels, g, dMax, vMax, pr, flow, nullptr, nullptr, minC);
}

fsgm_status fsgm_epipolar_flow_pp_host(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                       const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                       double* flow, double* flow2, double* D1, uint32_t* minC) {
    fsgm_epi_params pr;
    fsgm_status st = driver_args("fsgm_epipolar_flow_pp_host", true, n, I0, I1, W, H, channels, g, dMax, prm, flow, flow2, &pr);
    if (st != FSGM_OK) return st;
    return host_drive(true, n, I0, I1, W, H, channels, g, dMax, vMax, pr, flow, flow2, D1, minC);
}

// Device forms: the caller's arrays checked, the plan prepared before the join with the caller's stream, then on the plan's
// stream the caller's images as gray (:35-38, straight from its planes) and each frame's maps (:24, the geometry by value),
// with the caller's images and minC bound to the plan.
static fsgm_status device_drive(const char* who, bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H,
                                int32_t channels, const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                double* flow, double* flow2, double* D1, uint32_t* minC, void* stream, int32_t* status) {
    fsgm_epi_params pr;
    fsgm_status st = driver_args(who, pp, n, I0, I1, W, H, channels, g, dMax, prm, flow, flow2, &pr);
    if (st != FSGM_OK) return st;
    FSGM_DEVICE_SLOT(pr.device);
    if ((st = epi_plan_args(W, H, dMax, n, pr, FSGM_SAMPLING_VZ, 0)) != FSGM_OK) return st;
    const size_t NP = (size_t)W * H, np = (size_t)n * NP;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, pr.device, cs, {{I0, np * channels, 1, true, "I0"},
                                                     {I1, np * channels, 1, true, "I1"},
                                                     {flow, np * 24, 8, true, "flow"},
                                                     {pp ? flow2 : nullptr, np * 24, 8, pp, "flow2"},
                                                     {pp ? D1 : nullptr, np * 8, 8, false, "D1"},
                                                     {minC, np * 4, 4, false, "minC"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    if ((st = cached_plan(lk, &p, W, H, dMax, n, pr)) != FSGM_OK) return st;
    if ((st = ensure_driver_buffers(p, 1, pp)) != FSGM_OK) return st;
    if ((st = epi_device_prepare(p, 6, 64, vMax)) != FSGM_OK) return st;                 // epipolar_sgm_of.m:19, test.m:36
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, channels == 1 ? const_cast<uint8_t*>(I0) : nullptr), i2(p->dI2, channels == 1 ? const_cast<uint8_t*>(I1) : nullptr);
        Bind<uint32_t> mc(p->dMinC, minC);
        if (channels == 3) {
            launch_pyr_gray(p->stream, I0, p->dI1, W, H, n);
            launch_pyr_gray(p->stream, I1, p->dI2, W, H, n);
        }
        for (int f = 0; f < n; f++)
            launch_epi_maps(p->stream, geom_args(&g[f], W, H, p->dPd0 + f * 2 * NP, p->dNd + f * 2 * NP, p->dOff + f * NP, p->dRflow + f * 2 * NP));
        const fsgm_status es = enqueue_flow(p, pp, dMax, vMax, flow, flow2, D1 ? D1 : p->dD1);
        if (es == FSGM_OK) launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return es;
    });
}

fsgm_status fsgm_epipolar_sgm_of_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                        const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                        double* flow, uint32_t* minC, void* stream, int32_t* status) {
    return device_drive("fsgm_epipolar_sgm_of_device", false, n, I0, I1, W, H, channels, g, dMax, vMax, prm, flow, nullptr, nullptr, minC,
                        stream, status);
}

fsgm_status fsgm_epipolar_flow_pp_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                         const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                         double* flow, double* flow2, double* D1, uint32_t* minC, void* stream, int32_t* status) {
    return device_drive("fsgm_epipolar_flow_pp_device", true, n, I0, I1, W, H, channels, g, dMax, vMax, prm, flow, flow2, D1, minC,
                        stream, status);
}

}  // extern "C"
