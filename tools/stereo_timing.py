"""Device time of the rectified cost stage beside the general one, and of the whole stereo_sgm call, warm, at 1242x375x128.
Prints one JSON line.

  rect_cost_ms_per_frame[N]      FSGM_STAGE_COST of a rectified plan (census x2 + epi_costbox_kernel<8, rectified>), N frames,
                                 fsgm_epi_plan_time, divided by N (N = 1, 8, 40)
  general_cost_ms_per_frame[N]   the same stage of a vz-index plan on the same images with synth.epi_maps(kind="axis"): the
                                 general epi_costbox_kernel<8>, the yardstick
  linear_cost_ms_per_frame[N]    the same stage of a linear plan on the maps a rectified pair implies (the general kernel again)
  frac_of_8TBps[N]               (2 W H + W H D) bytes per frame / rect_cost_ms_per_frame against 8 TB/s
  host_call_ms[N]                fsgm_amd.stereo_sgm on N pairs from pageable numpy buffers, whole call, median wall time
  device_call_ms[N]              torch_ops.stereo_sgm on N pairs in HBM, median of events on the caller's stream
  rect_cost_ms_per_frame_d_min[d][N]   the d_min column (--d-mins 0,40): the rectified cost stage with the search range
                                 starting at d (fsgm_epi_plan_set_d_min), --repeats values each -- their spread is the
                                 run-to-run noise of this session.  A library without the entry point measures d = 0 only.
  range_gain                     (--range-gain) one pair, what a caller gains who knows the disparities lie in [40, 104): d_min =
                                 40, dMax = 64 against d_min = 0, dMax = 128 -- cost stage and the whole torch_ops.stereo_sgm call
  --only-rect                    no general / linear / whole-call columns (A/B runs of two builds of the library)

    python3 tools/stereo_timing.py [--iters 10] [--batches 1,8,40] [--d-mins 0,40] [--repeats 3] [--range-gain] [--only-rect]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import fsgm_amd  # noqa: E402
from fsgm_amd import EpiPlan, _lib, torch_ops, synth  # noqa: E402

DEV = "cuda:0"
W, H, D = 1242, 375, 128


def device_ms(fn, iters):
    s = torch.cuda.current_stream()
    fn()
    s.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def wall_ms(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def has_d_min():
    return hasattr(fsgm_amd.load_library(), "fsgm_epi_plan_set_d_min") and hasattr(EpiPlan, "set_d_min")


def cost_stage_ms(pairs, sampling, iters, d_min=0, dmax=D):
    n = len(pairs)
    with EpiPlan(W, H, dmax, n, sampling=sampling, direction=-1) as plan:
        plan.set_penalties(6, 64)
        if d_min:
            plan.set_d_min(d_min)
        if sampling == _lib.SAMPLING_RECTIFIED:
            for f, (I1, I2) in enumerate(pairs):
                plan.upload_images(f, I1, I2)
        else:
            pd0, nd, off = synth.epi_maps(W, H, "axis")
            for f, (I1, I2) in enumerate(pairs):
                plan.upload(f, I1, I2, pd0, nd, off)
        return plan.time(_lib.STAGE_COST, warmup=3, iters=iters) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,8,40")
    ap.add_argument("--d-mins", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--range-gain", action="store_true")
    ap.add_argument("--only-rect", action="store_true")
    a = ap.parse_args()
    d_mins = [int(d) for d in a.d_mins.split(",") if d != ""]
    if not has_d_min():
        d_mins = [d for d in d_mins if d == 0]
    batches = [int(b) for b in a.batches.split(",")]
    base = [synth.image_pair(W, H, D, seed=s) for s in range(1, 5)]
    out = {"shape": [W, H, D], "iters": a.iters, "paths": 4, "rect_cost_ms_per_frame": {}, "general_cost_ms_per_frame": {},
           "linear_cost_ms_per_frame": {}, "frac_of_8TBps": {}, "host_call_ms": {}, "device_call_ms": {}, "has_d_min": has_d_min()}
    if d_mins:
        out["rect_cost_ms_per_frame_d_min"] = {d: {} for d in d_mins}
    for n in batches:
        pairs = [tuple(np.roll(x, 7 * (f // len(base)), axis=1) for x in base[f % len(base)]) for f in range(n)]
        for _ in range(a.repeats):                               # (the columns interleaved: drift lands on all of them)
            for d in d_mins:
                out["rect_cost_ms_per_frame_d_min"][d].setdefault(n, []).append(cost_stage_ms(pairs, _lib.SAMPLING_RECTIFIED, a.iters, d))
        if a.only_rect:
            continue
        r = cost_stage_ms(pairs, _lib.SAMPLING_RECTIFIED, a.iters)
        out["rect_cost_ms_per_frame"][n] = r
        out["general_cost_ms_per_frame"][n] = cost_stage_ms(pairs, _lib.SAMPLING_VZ, a.iters)
        out["linear_cost_ms_per_frame"][n] = cost_stage_ms(pairs, _lib.SAMPLING_LINEAR, a.iters)
        out["frac_of_8TBps"][n] = (2.0 * W * H + 1.0 * W * H * D) / (r * 1e-3) / 8e12
        L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        out["host_call_ms"][n] = wall_ms(lambda: fsgm_amd.stereo_sgm(L, R, D), max(3, a.iters // 2))
        tL, tR = torch.from_numpy(L).to(DEV), torch.from_numpy(R).to(DEV)
        out["device_call_ms"][n] = device_ms(lambda: torch_ops.stereo_sgm(tL, tR, D), a.iters)
        fsgm_amd.load_library().fsgm_shutdown()                  # the cached plans of this batch size
    if a.range_gain and has_d_min():
        pair = base[:1]
        tL, tR = (torch.from_numpy(x[None]).to(DEV) for x in pair[0])
        g = {"cost_ms_d_min40_dmax64": [], "cost_ms_d_min0_dmax128": [], "call_ms_d_min40_dmax64": [], "call_ms_d_min0_dmax128": []}
        for _ in range(a.repeats):
            g["cost_ms_d_min40_dmax64"].append(cost_stage_ms(pair, _lib.SAMPLING_RECTIFIED, a.iters, 40, 64))
            g["cost_ms_d_min0_dmax128"].append(cost_stage_ms(pair, _lib.SAMPLING_RECTIFIED, a.iters, 0, 128))
            g["call_ms_d_min40_dmax64"].append(device_ms(lambda: torch_ops.stereo_sgm(tL, tR, 64, d_min=40), a.iters))
            g["call_ms_d_min0_dmax128"].append(device_ms(lambda: torch_ops.stereo_sgm(tL, tR, 128, d_min=0), a.iters))
        out["range_gain"] = g
    print(json.dumps(out))


if __name__ == "__main__":
    main()
