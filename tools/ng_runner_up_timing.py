"""Device time of a neighbour-guided level with the runner-up cost beside the level without it, warm, at 1242x375, and the
filtered-flow pipeline with a uniqueness ratio beside the plain one.

The level: a one-level NgPyramidPlan (one frame: census, costs, repeat removal, matcher, WTA) at D = 81 (halfSearchWinSize 1)
and D = 225 (halfSearchWinSize 2), fsgm_ng_pyramid_plan_time -- HIP events around the whole level on the plan's stream -- in two
states that alternate inside one run:
  off      the runner-up switch off (what every plain caller runs)
  on       the switch on: the WTA launch is the only one that differs, so on - off is what the runner-up WTA costs over the
           plain one (the events enclose the level, not the WTA alone: the library has no stage hook for this matcher)
The pipeline: fsgm_amd.pyramidal_flow_pp of one pair, both matchers, host wall clock of warm calls (uploads, the 2-frame level
loop, the chain, downloads), plain and with uniqueness_ratio=15.
The round is repeated; every figure of every round is printed (ms) and min / median / max per state, as JSON lines.  Against an
older build, run this tool once per build in interleaved processes with FSGM_LIB_PATH (an older build reports `off` alone).

    python3 tools/ng_runner_up_timing.py [--rounds 5] [--iters 30] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, synth  # noqa: E402

W, H = 1242, 375


def stats(ms):
    return {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in ms.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10, help="warm pipeline calls per state and round")
    a = ap.parse_args()
    lib = _lib.load()
    has_switch = hasattr(lib, "fsgm_ng_pyramid_plan_set_runner_up")
    I0, I1 = synth.image_pair(W, H, 16, seed=1)
    print(json.dumps({"shape": [W, H], "iters": a.iters, "rounds": a.rounds, "lib": _lib.LIB_PATH, "switch": has_switch}))
    for r in (1, 2):
        with fsgm_amd.NgPyramidPlan(W, H, 1, 1, halfSearchWinSize=r) as plan:
            plan.upload(I0, I1)
            plan.run()
            plan.download(1)
            ms = {"off": [], "on": []}
            for _ in range(a.rounds):
                if has_switch:
                    plan.set_runner_up(False)
                ms["off"].append(plan.time(3, a.iters))
                if has_switch:
                    plan.set_runner_up(True)
                    ms["on"].append(plan.time(3, a.iters))
        out = {"what": "level", "D": 9 * (2 * r + 1) ** 2, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items() if v},
               "min_median_max": stats(ms)}
        if ms["on"]:
            out["on_minus_off_ms"] = round(statistics.median(ms["on"]) - statistics.median(ms["off"]), 4)
        print(json.dumps(out), flush=True)
    for matcher in ("pyd", "ng"):
        ms = {"plain": [], "ratio": []}
        states = [("plain", {})] + ([("ratio", {"uniqueness_ratio": 15})] if has_switch else [])
        for _, kw in states:                                     # warm: the plans exist
            fsgm_amd.pyramidal_flow_pp(I0, I1, 3, matcher, **kw)
        for _ in range(a.rounds):
            for name, kw in states:
                t = time.perf_counter()
                for _ in range(a.calls):
                    fsgm_amd.pyramidal_flow_pp(I0, I1, 3, matcher, **kw)
                ms[name].append((time.perf_counter() - t) * 1e3 / a.calls)
        out = {"what": "pyramidal_flow_pp", "matcher": matcher, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items() if v},
               "min_median_max": stats(ms)}
        if ms["ratio"]:
            out["ratio_over_plain"] = round(statistics.median(ms["ratio"]) / statistics.median(ms["plain"]), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
