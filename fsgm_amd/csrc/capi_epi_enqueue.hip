// capi_epi_enqueue.hip -- what an epipolar plan queues (epi_plan.h: epi_enqueue, epi_tap_sum): the cost stage, each aggregation
// pipeline with its S debug tap, the WTA and the forward-backward check.  The choice among the pipelines and their buffers are
// capi_epi.hip's.
#include "epi_plan.h"
#include "epi_kernels.h"
#include "epi_view2.h"
#include <algorithm>

using namespace fsgm;

namespace {
// frame offset into a buffer the selected pipeline may not have
template <class T> T* frame_at(T* base, size_t off) { return base ? base + off : nullptr; }
}  // namespace

// Where the sweeps that meet in the middle meet: the row count of the down sweep's first half, a whole number of its launches
// (the up sweep's first half, H - hm rows, ends with a short launch).
static int meet_row(int H, int D) {
    const int t = 2 * sweep_rows_per_launch(D);                  // rows per launch of the 8-wave form
    const int hm = ((H + 1) / 2 + t - 1) / t * t;
    return std::min(hm, H);
}

// census x2 + cost fill + box of frames [f0, f0 + nf) on the plan's stream (epi_ensure_vz done by the caller)
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
    a.minC2 = p->runner_up ? p->dMinC2 + o : nullptr;            // (on: the plan is on the line kernels, epi_select_kernel)
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
fsgm_status fsgm::epi_enqueue(fsgm_epi_plan* p, int stages) {
    fsgm_status st = epi_prepare(p, stages);
    if (st != FSGM_OK) return st;
    if (stages & FSGM_STAGE_COST) {
        if ((st = epi_ensure_vz(p)) != FSGM_OK) return st;
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

// frame f's S into dS on the plan's stream, by the selected pipeline's tap
void fsgm::epi_tap_sum(fsgm_epi_plan* p, int f) {
    switch (p->pipe) {
        case PIPE_SWEEP: case PIPE_SWEEP_PAR: case PIPE_SWEEP_MID: tap_sweep(p, f); break;
        case PIPE_PAIRS: tap_pairs(p, f); break;
        case PIPE_BAND: case PIPE_BAND_CHAIN: tap_band(p, f); break;
        default: tap_lines(p, f); break;
    }
}
