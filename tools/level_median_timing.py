"""Device time of a whole pyramid run with the median between levels off, 3 and 5, warm, at 1242x375.

Both matchers at their default numPyd (pyramidal_sgm: 5, pyramidal_sgm_ng: 3), batch 1 and 8, one plan per matcher and batch:
fsgm_(ng_)pyramid_plan_time -- HIP events around the level loop on the plan's stream -- in three states that alternate inside
one run on the same plan:
  off      level_median 0 (what every plain caller runs)
  3, 5     the switch on: every level above the first makes the next level's hints by pyr_median_upsample2_kernel<S>; the pyd
           driver's pyr_flow_kernel then skips its own four stores, the ng driver's pyr_upsample2_kernel is not launched
The round is repeated; every figure of every round is printed (ms per run of the whole batch) and min / median / max per state,
as JSON lines, with on - off per pair.  Against an older build, run this tool once per build in interleaved processes with
FSGM_LIB_PATH (an older build reports `off` alone).

    python3 tools/level_median_timing.py [--rounds 5] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, synth  # noqa: E402

W, H = 1242, 375
PLANS = {"pyd": (fsgm_amd.PyramidPlan, 5), "ng": (fsgm_amd.NgPyramidPlan, 3)}


def stats(ms):
    return {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in ms.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    lib = _lib.load()
    has_switch = hasattr(lib, "fsgm_pyramid_plan_set_level_median")
    sizes = (0, 3, 5) if has_switch else (0,)
    print(json.dumps({"shape": [W, H], "iters": a.iters, "rounds": a.rounds, "lib": _lib.LIB_PATH, "switch": has_switch}))
    for matcher, (cls, numPyd) in PLANS.items():
        for batch in (1, 8):
            with cls(W, H, 1, numPyd, batch=batch) as plan:
                for f in range(batch):
                    plan.upload(*synth.image_pair(W, H, 16, seed=1 + f), frame=f)
                plan.run()
                plan.download(1)
                ms = {("off" if s == 0 else str(s)): [] for s in sizes}
                for _ in range(a.rounds):
                    for s in sizes:
                        if has_switch:
                            plan.set_level_median(s)
                        ms["off" if s == 0 else str(s)].append(plan.time(3, a.iters))
            out = {"matcher": matcher, "numPyd": numPyd, "batch": batch, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "min_median_max": stats(ms)}
            for s in sizes[1:]:
                out[f"on{s}_minus_off_ms_per_pair"] = round((statistics.median(ms[str(s)]) - statistics.median(ms["off"])) / batch, 4)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
