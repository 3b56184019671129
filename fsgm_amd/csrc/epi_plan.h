// epi_plan.h -- the device-resident plan behind the calc_cost_sgm entry points and what the epipolar capi_*.hip files share of it:
// capi_epi.hip (the plan, its buffers, its cache and the calc_cost_sgm one-shots), capi_epi_enqueue.hip (what a plan queues),
// capi_stereo.hip (rectified stereo), capi_sgm.hip (sgm(C) on caller-supplied volumes) and capi_epi_driver.hip (census, maps and
// the epipolar drivers).  Included by those five and by nothing else.
#pragma once
#include "capi_common.h"
#include "capi_device.h"
#include <mutex>
#include <vector>

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
inline bool pipe_exact(Pipeline k) { return k == PIPE_PACKED_EXACT || k == PIPE_GENERIC_EXACT; }
inline bool pipe_lines(Pipeline k) { return k <= PIPE_PACKED_WRAP || pipe_exact(k); }
inline bool pipe_sweep(Pipeline k) { return k == PIPE_SWEEP || k == PIPE_SWEEP_PAR || k == PIPE_SWEEP_MID; }

// The sub-forms of the selected pipeline, settled with it by epi_select_kernel: decisions only, never device pointers (the
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
    fsgm::DeviceJoin join;               // device-pointer entry points: the events that order the plan's stream with the caller's
    bool pinned = false;                 // a captured graph names this cached plan's buffers, stream and events: never evicted (PlanCache)
};

// the plan's second view as int32 true disparities for the length of one enqueue
struct View2Format {
    fsgm_epi_plan* p;
    View2Format(fsgm_epi_plan* q, int d_min) : p(q) { p->v2_add = (uint32_t)(256 * d_min); p->v2_marker = 0x80000000u; }
    ~View2Format() { p->v2_add = 0; p->v2_marker = 0xFFFFFFFFu; }
};

// (internal to the library: none of these is among its dynamic symbols)
#pragma GCC visibility push(hidden)
namespace fsgm {

// ---- capi_epi.hip ----
// what a plan can be refused for without a GPU, in fsgm_epi_plan_create_sampling's words
fsgm_status epi_plan_args(int W, int H, int D, int batch, const fsgm_epi_params& pr, int sampling, int direction);
// the options of an *_opts entry point (null: the defaults), checked
fsgm_status epi_read_options(const char* who, const fsgm_epi_options* opt, fsgm_epi_options* o);
// the pipeline and its sub-forms for the plan's shape, switches, penalties and cmax: called after any of them changes
void epi_select_kernel(fsgm_epi_plan* p);
// buffer sets created on first use: the cost stage's, the image pair alone, the S tap's, the one-shot entries' left-right check
// map, the epipolar drivers' (pp: test.m's frame body, host: its host form)
fsgm_status epi_ensure_cost_buffers(fsgm_epi_plan* p);
fsgm_status epi_ensure_image_buffers(fsgm_epi_plan* p);
fsgm_status epi_ensure_tap_buffers(fsgm_epi_plan* p);
fsgm_status epi_ensure_view2_conf(fsgm_epi_plan* p);
fsgm_status epi_ensure_driver_buffers(fsgm_epi_plan* p, int channels, bool pp = false, bool host = false);
fsgm_status epi_ensure_vz(fsgm_epi_plan* p);                     // the vz table of the plan's vMax, uploaded when it is stale
// what a run of `stages` needs before anything is queued: the switches' refusals, the kernel selection, the pipeline's buffers
fsgm_status epi_prepare(fsgm_epi_plan* p, int stages);
// a device call's first-call work (penalties, cost buffers, vz table, epi_prepare of every stage), ahead of the join with the caller's stream
fsgm_status epi_device_prepare(fsgm_epi_plan* p, int P1, int P2, double vMax);
// the chained band sweeps' give-up flag, read after a sync
fsgm_status epi_check_handoff(fsgm_epi_plan* p);

// ---- capi_epi_enqueue.hip ----
fsgm_status epi_enqueue(fsgm_epi_plan* p, int stages);           // epi_prepare, then the stages on the plan's streams (no synchronisation)
void epi_tap_sum(fsgm_epi_plan* p, int f);                       // frame f's S into dS on the plan's stream (epi_ensure_tap_buffers first)

// ---- the plan cache (capi_epi.hip) ----
// What the cache compares: callers that differ in any field never share a plan.  Of prm it compares paths, fb_check and vz_to_disp
// on prm.device; the plan found takes the rest of prm from the key.
struct EpiPlanKey {
    int W = 0, H = 0, D = 0, batch = 0;
    fsgm_epi_params prm = fsgm_epi_params_default();
    int sampling = FSGM_SAMPLING_VZ, direction = 0;              // direction: a rectified plan's, 0 otherwise
    int adaptive = 0, agg_mode = 0, runner_up = 0, exact = 0;
    int view2_dir = 0;                                           // the second view's direction, 0: the switch is off
};
// The cached plan of this key for an entry point: `lk` holds its device's lock for the length of the call, the device is current.
// must_exist: the call is being captured into a graph, where a plan cannot be created (FSGM_ERR_UNSUPPORTED without one).
fsgm_status cached_plan(std::unique_lock<std::mutex>& lk, fsgm_epi_plan** out, const EpiPlanKey& key, bool must_exist = false);

}  // namespace fsgm
#pragma GCC visibility pop
