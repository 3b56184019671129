// capi_epi.hip -- C ABI for the calc_cost_sgm path: the device-resident plan (epi_plan.h) -- its pipeline choice, its buffers,
// its methods -- the cache of plans behind every one-shot entry point of the epipolar families (cached_plan), and the
// calc_cost_sgm one-shots on host and device pointers (what the calc_cost_sgm mexFunction gateway calls).  See include/fsgm.h.
#include "epi_plan.h"
#include "epi_kernels.h"
#include "epi_view2.h"
#include "post_plan.h"
#include <algorithm>
#include <cmath>
#include <stdlib.h>
#include <string.h>

using namespace fsgm;

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

// The pipeline and its sub-forms, settled together: epi_enqueue() and the S tap read them and re-derive nothing.  The sub-form
// switches (A/B) are read here, once per process.
void fsgm::epi_select_kernel(fsgm_epi_plan* p) {
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
}  // namespace

// what a plan can be refused for without a GPU (pr: vz_to_disp already cleared for the samplings that have none); the device
// entry points that run on a cached plan ask this before they touch a device, as plan creation does
fsgm_status fsgm::epi_plan_args(int W, int H, int D, int batch, const fsgm_epi_params& pr, int sampling, int direction) {
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

// Buffers of the cost stage (census x2 -> raw costs -> box mean) and of everything else that reads the image pair or the
// coordinate maps: created together on first use, committed only when the whole set exists.
fsgm_status fsgm::epi_ensure_cost_buffers(fsgm_epi_plan* p) {
    if (p->dCraw) return FSGM_OK;                                // the set's own marker: created last
    const size_t B = p->batch;
    LazySet ls;
    ls.alloc(p->dI1, B * p->NP);                                 // (a slot that is filled already stays: epi_ensure_image_buffers)
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
fsgm_status fsgm::epi_ensure_image_buffers(fsgm_epi_plan* p) {
    if (p->dI1 && p->dI2) return FSGM_OK;
    LazySet ls;
    ls.alloc(p->dI1, (size_t)p->batch * p->NP);
    ls.alloc(p->dI2, (size_t)p->batch * p->NP);
    if (ls.err != hipSuccess) return lazy_fail(ls, "image buffers");
    ls.commit();
    return FSGM_OK;
}

fsgm_status fsgm::epi_ensure_vz(fsgm_epi_plan* p) {
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
fsgm_status fsgm::epi_check_handoff(fsgm_epi_plan* p) {
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
    return drain == 2 ? epi_check_handoff(p) : FSGM_OK;
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
fsgm_status fsgm::epi_prepare(fsgm_epi_plan* p, int stages) {
    if (p->adaptive && (stages & FSGM_STAGE_AGGREGATE)) {        // the aggregation reads I1 of every slot: refuse before anything is queued
        for (int f = 0; f < p->batch; f++)
            if (!p->dI1 || !p->have_img[f])
                return fail(FSGM_ERR_INVALID, "adaptive P2: no image uploaded for frame %d (fsgm_epi_plan_upload / _upload_images)", f);
    }
    if (p->view2 && (stages & FSGM_STAGE_COST) && p->sampling != FSGM_SAMPLING_RECTIFIED)
        return fail(FSGM_ERR_INVALID, "second view: the candidates of this plan's own cost stage share no line (upload the cost volumes instead)");
    if ((stages & FSGM_STAGE_COST) || p->prm.fb_check) {
        fsgm_status cs = epi_ensure_cost_buffers(p);
        if (cs != FSGM_OK) return cs;
    }
    if (stages & FSGM_STAGE_COST) {
        bool changed = false;
        for (int& c : p->cmax) { if (c != 24) changed = true; c = 24; }
        if (changed) epi_select_kernel(p);
    }
    if (stages & (FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) return ensure_agg_buffers(p);
    return FSGM_OK;
}

// the S tap's own buffers (one frame each), created on first use
fsgm_status fsgm::epi_ensure_tap_buffers(fsgm_epi_plan* p) {
    if (!p->dS) FSGM_HIP(hipMalloc((void**)&p->dS, p->N * 4));
    if (!p->dXup && (pipe_sweep(p->pipe) || p->pipe == PIPE_PAIRS)) FSGM_HIP(hipMalloc((void**)&p->dXup, p->N));
    return FSGM_OK;
}

// the one-shot entries' left-right check buffer [batch][NP]
fsgm_status fsgm::epi_ensure_view2_conf(fsgm_epi_plan* p) {
    if (!p->dConfV2) FSGM_HIP(hipMalloc((void**)&p->dConfV2, (size_t)p->batch * p->NP));
    return FSGM_OK;
}

// The epipolar drivers' buffers (RGB staging: host forms with RGB planes); test.m's frame body (pp) also has the
// post-processing chain's scratch plan and D1, and its host form flow2.
fsgm_status fsgm::epi_ensure_driver_buffers(fsgm_epi_plan* p, int channels, bool pp, bool host) {
    { fsgm_status cs = epi_ensure_cost_buffers(p); if (cs != FSGM_OK) return cs; }
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

// the options of an *_opts entry point (null: the defaults), checked
fsgm_status fsgm::epi_read_options(const char* who, const fsgm_epi_options* opt, fsgm_epi_options* o) {
    *o = opt ? *opt : fsgm_epi_options_default();
    FSGM_REQUIRE(o->adaptive_p2 == 0 || o->adaptive_p2 == 1, "%s: adaptive_p2 must be 0 or 1 (got %d)", who, o->adaptive_p2);
    for (int r : o->reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_epi_options must be zero", who);
    return FSGM_OK;
}

extern "C" {

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
    // on first use (epi_ensure_cost_buffers): an aggregation-only plan holds C, the offsets and its pipeline's volumes only
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
    epi_select_kernel(p);
    *out = p;
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_penalties(fsgm_epi_plan* p, int32_t P1, int32_t P2, double vMax) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(!p->exact || (P1 >= 0 && P1 <= 255 && P2 >= 0 && P2 <= 255),
                 "fsgm_epi_plan_set_penalties: an exact plan takes P1 and P2 in 0..255 (got %d, %d)", P1, P2);
    p->P1 = P1; p->P2 = P2;
    if (vMax != p->vMax) p->vz_valid = false;
    p->vMax = vMax;
    epi_select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_upload(fsgm_epi_plan* p, int32_t f, const uint8_t* I1, const uint8_t* I2,
                                 const double* pd0, const double* nd, const double* off) {
    FSGM_REQUIRE(p, "null plan");
    { fsgm_status fs = frame_ready(p, f, 0); if (fs != FSGM_OK) return fs; }
    FSGM_REQUIRE(p->sampling != FSGM_SAMPLING_RECTIFIED, "fsgm_epi_plan_upload: a rectified plan takes images only (fsgm_epi_plan_upload_images)");
    FSGM_REQUIRE(I1 && I2 && pd0 && nd && (off || p->sampling == FSGM_SAMPLING_LINEAR), "fsgm_epi_plan_upload: null input");
    { fsgm_status cs = epi_ensure_cost_buffers(p); if (cs != FSGM_OK) return cs; }
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
    { fsgm_status cs = epi_ensure_image_buffers(p); if (cs != FSGM_OK) return cs; }   // (the cost stage's other buffers: epi_prepare())
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
    epi_select_kernel(p);
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
    epi_select_kernel(p);
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

fsgm_status fsgm_epi_plan_run(fsgm_epi_plan* p, int32_t stages) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE((stages & ~FSGM_STAGE_ALL) == 0 && stages != 0, "bad stage mask %d", stages);
    FSGM_HIP(hipSetDevice(p->prm.device));
    return epi_enqueue(p, stages);
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
    epi_select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_adaptive_p2(fsgm_epi_plan* p, int32_t on) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_adaptive_p2: on must be 0 or 1 (got %d)", on);
    if (on && p->agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "adaptive P2 on a plan forced to agg mode %d: only the line kernels (modes 0 and 1) take a per-step P2",
                    p->agg_mode);
    p->adaptive = on;
    epi_select_kernel(p);
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
    epi_select_kernel(p);
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
    epi_select_kernel(p);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_set_view2(fsgm_epi_plan* p, int32_t on, int32_t direction) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "fsgm_epi_plan_set_view2: on must be 0 or 1 (got %d)", on);
    if (!on) { p->view2 = 0; epi_select_kernel(p); return FSGM_OK; }
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
    epi_select_kernel(p);
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

fsgm_status fsgm_epi_plan_download_sum(fsgm_epi_plan* p, int32_t f, uint32_t* S) {
    FSGM_REQUIRE(p && S, "fsgm_epi_plan_download_sum: null argument");
    { fsgm_status fs = frame_ready(p, f, 2); if (fs != FSGM_OK) return fs; }
    // the line kernels sum the frame's path volumes; the fused pipelines never hold S in HBM and rebuild it (tap_*)
    { fsgm_status es = ensure_agg_buffers(p); if (es != FSGM_OK) return es; }
    { fsgm_status es = epi_ensure_tap_buffers(p); if (es != FSGM_OK) return es; }
    epi_tap_sum(p, f);
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
    const fsgm_status st = time_enqueues(p->stream, p->ev0, p->ev1, warmup, iters, [&] { return epi_enqueue(p, stages); }, ms_avg);
    if (st != FSGM_OK) return st;
    return epi_check_handoff(p);                                     // a timed run that gave up on a hand-off is not a measurement
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

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// host-pointer entry points (the MEX boundary).  Plans are cached per shape for the lifetime of
// the process so repeated MEX calls do not re-allocate HBM (SURVEY 8b "ownership").
// ---------------------------------------------------------------------------------------------
// cached plans per device (the cap bounds the HBM held by stale shapes; a plan recorded into a graph is held beside them)
static PlanCache<fsgm_epi_plan> g_epi(4, fsgm_epi_plan_destroy, [](const fsgm_epi_plan* p) { return p->pinned; });

// whether cached plan q serves a caller with key k
// (a plan serves one sampling mode and, rectified, one direction: the modes share no cached state)
static bool plan_has_key(const fsgm_epi_plan* q, const EpiPlanKey& k) {
    return q->W == k.W && q->H == k.H && q->D == k.D && q->batch == k.batch && q->prm.paths == k.prm.paths &&
           q->prm.fb_check == k.prm.fb_check && q->prm.vz_to_disp == k.prm.vz_to_disp && q->sampling == k.sampling &&
           q->direction == k.direction && q->adaptive == k.adaptive &&   // (adaptive and non-adaptive callers never share a plan)
           q->agg_mode == k.agg_mode &&                                  // (nor do forced modes: only the sgm batch forms ask for one)
           q->runner_up == k.runner_up &&                                // (nor a runner-up caller and a plain one: the plain call keeps its pipeline)
           q->exact == k.exact &&                                        // (nor an exact caller and a plain one)
           q->view2 == (k.view2_dir != 0) && (!k.view2_dir || q->v2_dir == k.view2_dir);   // (nor a second-view caller and a plain one)
}

// the key's switches on a fresh plan, each one that is on, in this order, up to the first that is refused
static fsgm_status set_key_switches(fsgm_epi_plan* p, const EpiPlanKey& k) {
    fsgm_status st = FSGM_OK;
    if (k.adaptive && (st = fsgm_epi_plan_set_adaptive_p2(p, 1)) != FSGM_OK) return st;
    if (k.agg_mode && (st = fsgm_epi_plan_set_agg_mode(p, k.agg_mode)) != FSGM_OK) return st;
    if (k.runner_up && (st = fsgm_epi_plan_set_runner_up(p, 1)) != FSGM_OK) return st;
    if (k.exact && (st = fsgm_epi_plan_set_exact(p, 1)) != FSGM_OK) return st;
    if (k.view2_dir && (st = fsgm_epi_plan_set_view2(p, 1, k.view2_dir)) != FSGM_OK) return st;
    return st;
}

fsgm_status fsgm::cached_plan(std::unique_lock<std::mutex>& lk, fsgm_epi_plan** out, const EpiPlanKey& k, bool must_exist) {
    const fsgm_epi_params& pr = k.prm;
    FSGM_DEVICE_SLOT(pr.device);
    lk = std::unique_lock<std::mutex>(g_epi.mu(pr.device));
    fsgm_epi_plan* p = g_epi.find(pr.device, [&](const fsgm_epi_plan* q) { return plan_has_key(q, k); });
    if (p) p->prm = pr;
    else if (must_exist)                                         // (a captured call: creating a plan allocates, copies and waits)
        return fail(FSGM_ERR_UNSUPPORTED, "the stream is being captured into a graph and no call of this shape and these switches has run yet: "
                                          "run it once outside the capture");
    else {
        fsgm_status st = fsgm_epi_plan_create_sampling(&p, k.W, k.H, k.D, k.batch, &pr, k.sampling, k.direction);
        if (st == FSGM_OK && (st = set_key_switches(p, k)) != FSGM_OK) fsgm_epi_plan_destroy(p);
        if (st != FSGM_OK) return st;
        g_epi.insert(pr.device, p);
    }
    *out = p;
    FSGM_HIP(hipSetDevice(pr.device));
    return FSGM_OK;
}

extern "C" __attribute__((visibility("hidden"))) void fsgm_epi_shutdown_internal(void) { g_epi.clear(); }   // fsgm_shutdown's hook (capi_runtime.hip)

// calc_cost_sgm on host pointers in either build of the reference: vz-index sampling, or linear (offset and vMax unused)
static fsgm_status epi_batch_host(int sampling, int32_t n, const fsgm_epi_in* in, const fsgm_epi_out* out, const fsgm_epi_params* prm,
                                  const fsgm_epi_options* opt) {
    FSGM_REQUIRE(n >= 1 && in && out, "fsgm_calc_cost_sgm: null argument");
    fsgm_epi_options o;
    { const fsgm_status os = epi_read_options("fsgm_calc_cost_sgm", opt, &o); if (os != FSGM_OK) return os; }
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
    EpiPlanKey key;
    key.W = in[0].width; key.H = in[0].height; key.D = in[0].dMax; key.batch = n; key.prm = pr;
    key.sampling = sampling; key.adaptive = o.adaptive_p2;
    fsgm_status st = cached_plan(lk, &p, key);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, in[0].P1, in[0].P2, linear ? p->vMax : in[0].vMax)) != FSGM_OK) return st;
    if ((st = epi_ensure_cost_buffers(p)) != FSGM_OK) return st;
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
    if ((st = epi_enqueue(p, FSGM_STAGE_ALL)) != FSGM_OK) return st;
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
    if ((st = epi_check_handoff(p)) != FSGM_OK) return st;
    if (taps)
        for (int i = 0; i < n; i++)
            if (out[i].S && (st = fsgm_epi_plan_download_sum(p, i, out[i].S)) != FSGM_OK) return st;
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
fsgm_status fsgm::epi_device_prepare(fsgm_epi_plan* p, int P1, int P2, double vMax) {
    fsgm_status st;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, vMax)) != FSGM_OK) return st;
    if ((st = epi_ensure_cost_buffers(p)) != FSGM_OK) return st;
    if ((st = epi_ensure_vz(p)) != FSGM_OK) return st;
    p->have_img.assign(p->batch, 1);                             // the caller's images stand in for the plan's for this enqueue
    return epi_prepare(p, FSGM_STAGE_ALL);
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
        if ((st = epi_read_options(who, opt, &o)) != FSGM_OK) return st;
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
    EpiPlanKey key;
    key.W = in->width; key.H = in->height; key.D = in->dMax; key.batch = n; key.prm = pr;
    key.sampling = sampling; key.adaptive = o.adaptive_p2;
    if (!p && (st = cached_plan(lk, &p, key)) != FSGM_OK) return st;
    if ((st = epi_device_prepare(p, in->P1, in->P2, linear ? p->vMax : in->vMax)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, const_cast<uint8_t*>(in->I1)), i2(p->dI2, const_cast<uint8_t*>(in->I2));
        Bind<double> pd0(p->dPd0, const_cast<double*>(in->pixelPosD0)), nd(p->dNd, const_cast<double*>(in->normDir));
        Bind<double> off(p->dOff, linear ? nullptr : const_cast<double*>(in->offset));   // (linear: the plan's own 1.0 map)
        Bind<uint32_t> bd(p->dBestD, out->bestD), mc(p->dMinC, out->minC), d2(p->dD2, fb ? out->bestD2 : nullptr);
        Bind<uint8_t> conf(p->dConf, fb ? out->conf : nullptr);
        const fsgm_status es = epi_enqueue(p, FSGM_STAGE_ALL);
        if (es == FSGM_OK) launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return es;
    });
}

extern "C" {

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

}  // extern "C"
