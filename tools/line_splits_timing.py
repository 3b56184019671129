"""Device time of aggregation + WTA at the disparity ranges of the 12-costs-a-lane split (48, 96, 192), warm, at 1242x375.

For 1 and 8 frames at 4 and 8 paths, fsgm_epi_plan_time(FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA) of one plan per dMax, auto mode.
The plans of a (paths, frames) point are created together and alternate inside one run; the round is repeated and every figure
of every round is printed (ms per batch), as JSON lines, with the pipeline each plan reports.  --controls adds the neighbouring
16 << k ranges (64, 128, 256), which take the same kernels in every build: they show whether two runs are comparable.

With FSGM_LIB_PATH pointing at a build from before agg_line_split() the same command times the generic kernels at the same
shapes -- the yardstick.  --compare NEW OLD reads two such outputs and prints, per point, the new build's median and spread, the
old build's, and whether new is faster than old by more than old's own round-to-round spread (max - min) in that run.

    python3 tools/line_splits_timing.py [--rounds 5] [--iters 10] [--batches 1,8] [--paths 4,8] [--dmax 48,96,192] [--controls]
    python3 tools/line_splits_timing.py --compare new.jsonl old.jsonl

On a shared device run each invocation under its own time limit and chain them with &&.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1242, 375


def measure(a):
    from fsgm_amd import EpiPlan, _lib, synth
    stages = _lib.STAGE_AGGREGATE | _lib.STAGE_WTA
    _lib.load()
    ranges = [int(d) for d in a.dmax.split(",")] + ([64, 128, 256] if a.controls else [])
    vols = {D: synth.cost_volume(W, H, D, seed=3, cmax=24) for D in ranges}
    _, _, off = synth.epi_maps(W, H, "axis")
    print(json.dumps({"shape": [W, H], "dmax": ranges, "stages": "aggregate+wta", "iters": a.iters, "rounds": a.rounds,
                      "lib": _lib.LIB_PATH}), flush=True)
    for paths in [int(p) for p in a.paths.split(",")]:
        for n in [int(b) for b in a.batches.split(",")]:
            plans = {}
            try:
                for D in ranges:
                    plans[D] = plan = EpiPlan(W, H, D, n, paths=paths)
                    plan.set_penalties(6, 64)
                    plan.upload_cost(0, vols[D])
                    for f in range(n):
                        if f:
                            plan.copy_cost(f, 0, 7 * f)
                        plan.upload_offset(f, off)
                ms = {D: [] for D in ranges}
                for _ in range(a.rounds):
                    for D in ranges:                             # the states alternate inside a round
                        ms[D].append(plans[D].time(stages, warmup=3, iters=a.iters))
                for D in ranges:
                    print(json.dumps({"paths": paths, "frames": n, "dmax": D, "kernel": plans[D].kernel_name,
                                      "ms": [round(x, 4) for x in ms[D]], "median_ms": round(statistics.median(ms[D]), 4)}), flush=True)
            finally:
                for plan in plans.values():
                    plan.close()


def compare(new_path, old_path):
    def points(path):
        out = {}
        for line in open(path):
            line = line.strip()
            if line.startswith("{") and '"ms"' in line:
                r = json.loads(line)
                out[(r["dmax"], r["frames"], r["paths"])] = r
        return out
    new, old = points(new_path), points(old_path)
    print("| dMax | frames | paths | new: pipeline | new: median (min .. max) ms | old: pipeline | old: median (min .. max) ms | old / new | faster by more than old's spread |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in sorted(new):
        if key not in old:
            continue
        n, o = new[key], old[key]
        spread = max(o["ms"]) - min(o["ms"])
        ok = o["median_ms"] - n["median_ms"] > spread and max(n["ms"]) < min(o["ms"])
        print(f"| {key[0]} | {key[1]} | {key[2]} | {n['kernel']} | {n['median_ms']:.3f} ({min(n['ms']):.3f} .. {max(n['ms']):.3f}) | {o['kernel']} | "
              f"{o['median_ms']:.3f} ({min(o['ms']):.3f} .. {max(o['ms']):.3f}) | {o['median_ms'] / n['median_ms']:.2f} | {'yes' if ok else 'NO'} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--paths", default="4,8")
    ap.add_argument("--dmax", default="48,96,192")
    ap.add_argument("--controls", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("NEW", "OLD"))
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
    else:
        measure(a)


if __name__ == "__main__":
    main()
