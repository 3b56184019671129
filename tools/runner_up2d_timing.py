"""Device time of the 2-D matcher's WTA stage with the runner-up cost beside the WTA without it, warm, at 1242x375.

For a 9x9 window (pyd_rows_wta_kernel<3>) and a 13x13 window (pyd_wta_kernel, above the row-packed limit), one frame,
fsgm_pyd_plan_time(FSGM_STAGE_WTA) of a plan whose path volumes are in place, in up to three states that alternate inside one run:
  off      the runner-up switch off (what every plain caller runs)
  on       the switch on (the second masked minimum and 4 more bytes per pixel)
  parent   an older build of the library named by --parent / FSGM_LIB_PATH_PARENT, which has no switch -- the A/B of the one
           condition that binds: `off` of this build must lie within the parent's own min-to-max spread of the same run
The round is repeated; every figure of every round is printed (ms) and min / median / max per state, as JSON lines.  Both
libraries live in this one process, each with a plan of its own over the same image pair.

    python3 tools/runner_up2d_timing.py [--rounds 5] [--iters 50] [--windows 4,6] [--parent /path/to/older/libfsgm_hip.so] [--parent-first]
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

W, H = 1242, 375


class Plan:
    """a one-frame plan through the C ABI of `lib` (either build), all stages run once"""

    def __init__(self, lib, half, I1, I2, mv):
        self.lib, self.h = lib, C.c_void_p()
        vp, i32 = C.c_void_p, C.c_int32
        lib.fsgm_pyd_plan_create.argtypes = [C.POINTER(vp)] + [i32] * 9
        lib.fsgm_pyd_plan_destroy.argtypes, lib.fsgm_pyd_plan_destroy.restype = [vp], None
        lib.fsgm_pyd_plan_set_params.argtypes = [vp] + [i32] * 6
        lib.fsgm_pyd_plan_upload.argtypes = [vp, i32, vp, vp, vp]
        lib.fsgm_pyd_plan_run.argtypes = [vp, i32]
        lib.fsgm_pyd_plan_download.argtypes = [vp, i32, vp, vp, vp]
        lib.fsgm_pyd_plan_time.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
        lib.fsgm_last_error.restype = C.c_char_p
        self.ok(lib.fsgm_pyd_plan_create(C.byref(self.h), W, H, W, H, half, half, 2, 1, 0))
        self.ok(lib.fsgm_pyd_plan_set_params(self.h, 6, 32, 1, 2, 0, 1))
        self.ok(lib.fsgm_pyd_plan_upload(self.h, 0, _lib.ptr(I1), _lib.ptr(I2), _lib.ptr(mv)))
        self.ok(lib.fsgm_pyd_plan_run(self.h, _lib.STAGE_ALL))   # the path volumes the WTA reads
        self.ok(lib.fsgm_pyd_plan_download(self.h, 0, None, None, None))   # (waits for the stream)

    def ok(self, st):
        if st != 0:
            raise RuntimeError(f"fsgm status {st}: {self.lib.fsgm_last_error().decode()}")

    def switch(self, on):
        self.lib.fsgm_pyd_plan_set_runner_up.argtypes = [C.c_void_p, C.c_int32]
        self.ok(self.lib.fsgm_pyd_plan_set_runner_up(self.h, on))

    def time_wta(self, iters):
        ms = C.c_float()
        self.ok(self.lib.fsgm_pyd_plan_time(self.h, _lib.STAGE_WTA, 3, iters, C.byref(ms)))
        return float(ms.value)

    def close(self):
        self.lib.fsgm_pyd_plan_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", default="4,6", help="half sizes: 4 is 9x9, 6 is 13x13")
    ap.add_argument("--parent", default=os.environ.get("FSGM_LIB_PATH_PARENT", ""))
    ap.add_argument("--parent-first", action="store_true", help="create the parent's plan ahead of this build's (default: after it)")
    a = ap.parse_args()
    child = _lib.load()
    parent = C.CDLL(a.parent) if a.parent else None
    I1, I2 = synth.image_pair(W, H, 16, seed=1)
    mv = np.ascontiguousarray(synth.hint_map(W, H, "general", seed=5, amp=3.0))
    print(json.dumps({"shape": [W, H], "stage": "wta", "iters": a.iters, "rounds": a.rounds, "lib": _lib.LIB_PATH, "parent": a.parent or None}))
    for half in [int(b) for b in a.windows.split(",")]:
        old = Plan(parent, half, I1, I2, mv) if parent and a.parent_first else None
        plan = Plan(child, half, I1, I2, mv)
        if parent and not a.parent_first:
            old = Plan(parent, half, I1, I2, mv)
        ms = {"off": [], "on": [], "parent": []}
        has_switch = hasattr(child, "fsgm_pyd_plan_set_runner_up")   # (FSGM_LIB_PATH on an older build: `off` alone)
        for _ in range(a.rounds):
            if has_switch:
                plan.switch(0)
            ms["off"].append(plan.time_wta(a.iters))
            if has_switch:
                plan.switch(1)
                ms["on"].append(plan.time_wta(a.iters))
            if old:
                ms["parent"].append(old.time_wta(a.iters))
        out = {"window": f"{2 * half + 1}x{2 * half + 1}", "created_first": "parent" if old and a.parent_first else "this build", "ms": {k: [round(x, 4) for x in v] for k, v in ms.items() if v},
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
