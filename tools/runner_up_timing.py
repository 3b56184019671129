"""Device time of the line kernels' WTA with the runner-up cost beside the WTA without it, warm, at 1242x375x128, 8 paths.

For 1 and 8 frames, fsgm_epi_plan_time(FSGM_STAGE_WTA) of a plan forced to the line kernels (mode 1), in up to three states that
alternate inside one run:
  off      the runner-up switch off (wta_packed_kernel<8>: what every plain caller runs)
  on       the switch on (wta_packed_ru_kernel<8>: a second masked minimum and 4 more bytes per pixel)
  parent   an older build of the library named by FSGM_LIB_PATH_PARENT, switch off only -- the A/B of the one condition that
           binds: `off` of this build must lie within the parent's own min-to-max spread of the same run
The round is repeated; every figure of every round is printed (ms per batch) and min / median / max per state at the end, as
JSON lines.  Both libraries live in this one process, each with plans of its own over the same volumes.

    python3 tools/runner_up_timing.py [--rounds 5] [--iters 50] [--batches 1,8] [--parent /path/to/older/libfsgm_hip.so]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from fsgm_amd import _lib, synth  # noqa: E402

W, H, D, PATHS = 1242, 375, 128, 8
AGG, WTA = _lib.STAGE_AGGREGATE, _lib.STAGE_WTA


class Plan:
    """an aggregation-only plan of `n` frames through the C ABI of `lib` (either build), forced to the line kernels"""

    def __init__(self, lib, n, Cv):
        self.lib, self.h = lib, C.c_void_p()
        vp, i32 = C.c_void_p, C.c_int32
        lib.fsgm_epi_plan_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, C.POINTER(_lib.EpiParams)]
        lib.fsgm_epi_plan_destroy.argtypes, lib.fsgm_epi_plan_destroy.restype = [vp], None
        lib.fsgm_epi_plan_set_penalties.argtypes = [vp, i32, i32, C.c_double]
        lib.fsgm_epi_plan_set_agg_mode.argtypes = [vp, i32]
        lib.fsgm_epi_plan_upload_cost.argtypes = [vp, i32, vp]
        lib.fsgm_epi_plan_copy_cost.argtypes = [vp, i32, i32, i32]
        lib.fsgm_epi_plan_run.argtypes = [vp, i32]
        lib.fsgm_epi_plan_sync.argtypes = [vp]
        lib.fsgm_epi_plan_time.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
        lib.fsgm_epi_plan_kernel_name.argtypes, lib.fsgm_epi_plan_kernel_name.restype = [vp], C.c_char_p
        lib.fsgm_last_error.restype = C.c_char_p
        prm = _lib.EpiParams(PATHS, 1, 0, 0, 0)
        self.ok(lib.fsgm_epi_plan_create(C.byref(self.h), W, H, D, n, C.byref(prm)))
        self.ok(lib.fsgm_epi_plan_set_penalties(self.h, 6, 64, 0.3))
        self.ok(lib.fsgm_epi_plan_upload_cost(self.h, 0, _lib.ptr(Cv)))
        for f in range(1, n):
            self.ok(lib.fsgm_epi_plan_copy_cost(self.h, f, 0, 7 * f))
        self.ok(lib.fsgm_epi_plan_set_agg_mode(self.h, 1))
        self.ok(lib.fsgm_epi_plan_run(self.h, AGG | WTA))        # the path volumes the WTA reads
        self.ok(lib.fsgm_epi_plan_sync(self.h))

    def ok(self, st):
        if st != 0:
            raise RuntimeError(f"fsgm status {st}: {self.lib.fsgm_last_error().decode()}")

    def switch(self, on):
        self.lib.fsgm_epi_plan_set_runner_up.argtypes = [C.c_void_p, C.c_int32]
        self.ok(self.lib.fsgm_epi_plan_set_runner_up(self.h, on))

    def time_wta(self, iters):
        ms = C.c_float()
        self.ok(self.lib.fsgm_epi_plan_time(self.h, WTA, 3, iters, C.byref(ms)))
        return float(ms.value)

    def name(self):
        return self.lib.fsgm_epi_plan_kernel_name(self.h).decode()

    def close(self):
        self.lib.fsgm_epi_plan_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--parent", default=os.environ.get("FSGM_LIB_PATH_PARENT", ""))
    a = ap.parse_args()
    child = _lib.load()
    parent = C.CDLL(a.parent) if a.parent else None
    Cv = np.ascontiguousarray(synth.cost_volume(W, H, D, seed=3, cmax=24))
    print(json.dumps({"shape": [W, H, D], "paths": PATHS, "stage": "wta", "iters": a.iters, "rounds": a.rounds, "lib": _lib.LIB_PATH,
                      "parent": a.parent or None}))
    for n in [int(b) for b in a.batches.split(",")]:
        plan = Plan(child, n, Cv)
        old = Plan(parent, n, Cv) if parent else None
        ms = {"off": [], "on": [], "parent": []}
        has_switch = hasattr(child, "fsgm_epi_plan_set_runner_up")   # (FSGM_LIB_PATH on an older build: `off` alone)
        for _ in range(a.rounds):
            if has_switch:
                plan.switch(0)
            ms["off"].append(plan.time_wta(a.iters))
            if has_switch:
                plan.switch(1)
                ms["on"].append(plan.time_wta(a.iters))
            if old:
                ms["parent"].append(old.time_wta(a.iters))
        out = {"frames": n, "kernel": plan.name(), "ms": {k: [round(x, 4) for x in v] for k, v in ms.items() if v},
               "min_median_max": {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in ms.items() if v},
               "on_over_off": round(statistics.median(ms["on"]) / statistics.median(ms["off"]), 3) if ms["on"] else None}
        if old:
            med = statistics.median(ms["off"])
            out["off_within_parent_spread"] = bool(min(ms["parent"]) <= med <= max(ms["parent"]))
            old.close()
        plan.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
