"""Device time of aggregation + WTA with adaptive P2 beside the non-adaptive line kernels and auto mode, warm, at 1242x375x128.

For 1, 8 and 40 frames at 4 and 8 paths, fsgm_epi_plan_time(FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA) of one plan in three states:
  adaptive      adaptive P2 on (the general body of the line kernels with a pixel ring, every batch size)
  lines         adaptive off, aggregation mode 1 (the line kernels as they are without the switch: the hand-written bodies)
  auto          adaptive off, mode 0 (what a non-adaptive caller gets: line kernels, sweeps or pairs by batch size)
The three alternate inside one run and the round is repeated; every figure of every round is printed (ms per batch) and the
median per state at the end, as JSON lines.  With a library that has no adaptive switch (FSGM_LIB_PATH pointing at an older
build, for an A/B of the non-adaptive times) the `adaptive` state is left out.

    python3 tools/adaptive_p2_timing.py [--rounds 5] [--iters 20] [--batches 1,8,40] [--paths 4,8]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from fsgm_amd import EpiPlan, _lib, synth  # noqa: E402

W, H, D = 1242, 375, 128
STAGES = _lib.STAGE_AGGREGATE | _lib.STAGE_WTA


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,8,40")
    ap.add_argument("--paths", default="4,8")
    a = ap.parse_args()
    lib = _lib.load()
    has_switch = hasattr(lib, "fsgm_epi_plan_set_adaptive_p2")
    Cv = synth.cost_volume(W, H, D, seed=3, cmax=24)
    I1, I2 = synth.image_pair(W, H, D, seed=1)
    _, _, off = synth.epi_maps(W, H, "axis")
    print(json.dumps({"shape": [W, H, D], "stages": "aggregate+wta", "iters": a.iters, "rounds": a.rounds, "lib": _lib.LIB_PATH,
                      "edge_share_along_x": float((abs(I1[:, 1:].astype(int) - I1[:, :-1].astype(int)) > 25).mean())}))
    for paths in [int(p) for p in a.paths.split(",")]:
        for n in [int(b) for b in a.batches.split(",")]:
            with EpiPlan(W, H, D, n, paths=paths) as plan:
                plan.set_penalties(6, 64)
                plan.upload_cost(0, Cv)
                plan.upload_offset(0, off)
                if has_switch:
                    plan.upload_images(0, I1, I2)
                for f in range(1, n):
                    plan.copy_cost(f, 0, 7 * f)
                    plan.upload_offset(f, off)
                    if has_switch:
                        plan.upload_images(f, np.roll(I1, 7 * f, axis=1), I2)
                ms, names = {"adaptive": [], "lines": [], "auto": []}, {}
                for _ in range(a.rounds):
                    for state in ("adaptive", "lines", "auto"):
                        if state == "adaptive":
                            if not has_switch:
                                continue
                            plan.set_agg_mode(0)
                            plan.set_adaptive_p2(1)
                        else:
                            if has_switch:
                                plan.set_adaptive_p2(0)
                            plan.set_agg_mode(1 if state == "lines" else 0)
                        ms[state].append(plan.time(STAGES, warmup=3, iters=a.iters))
                        names[state] = plan.kernel_name
                print(json.dumps({"paths": paths, "frames": n, "kernel": names,
                                  "ms": {k: [round(x, 4) for x in v] for k, v in ms.items() if v},
                                  "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items() if v}}), flush=True)


if __name__ == "__main__":
    main()
