"""Device time of sgm2d(C) with exact path arithmetic beside the plain (mod-256) call of the same build, warm, on 1242x375
volumes of random bytes with 9x9 and 13x13 windows, P1 = 7, P2 = 100: the case the exact mode exists for, where the plain call
runs "generic/wrap".

For each window and 1 and 8 frames, three states on tensors in HBM, interleaved in one process, each timed by a pair of events on
the caller's stream around `iters` back-to-back calls (ingest, aggregation, WTA):

  wrap     fsgm_sgm2d_device on the random bytes                       "generic/wrap"
  exact    fsgm_sgm2d_device_exact on the same bytes                   "generic/exact"
  rows     (9x9 only, for context) fsgm_sgm2d_device on costs <= 24 at P1 = 6, P2 = 32, cost_bound 24: inside the no-wrap
           budget, the row-packed aggregation -- what a row-packed exact aggregation would have to be measured against

The comparison that matters is exact against wrap: the step masks less, the WTA reads ndirs + 1 volumes where it read ndirs.
Every figure of every round is printed (ms per call) and min / median / max per state at the end, as JSON lines.

    python3 tools/sgm2d_exact_timing.py [--rounds 5] [--iters 10] [--batches 1,8] [--windows 4,6]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # noqa: I001 -- first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsgm_amd import torch_ops  # noqa: E402
from fsgm_amd.sgm2d import last_kernel  # noqa: E402

W, H, P1, P2 = 1242, 375, 7, 100


def timed(call, iters):
    """ms per call of `iters` back-to-back calls on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--windows", default="4,6", help="half sizes: 4 = 9x9, 6 = 13x13")
    a = ap.parse_args()
    print(json.dumps({"shape": [W, H], "P1": P1, "P2": P2, "costs": "uniform random bytes", "iters": a.iters, "rounds": a.rounds}))
    g = torch.Generator(device="cuda").manual_seed(3)
    for r in [int(w) for w in a.windows.split(",")]:
        D = (2 * r + 1) ** 2
        for n in [int(b) for b in a.batches.split(",")]:
            Cv = torch.randint(0, 256, (n, D, H, W), dtype=torch.uint8, device="cuda", generator=g)
            calls = {"wrap": lambda: torch_ops.sgm2d(Cv, r, r, P1, P2, layout="dhw"),
                     "exact": lambda: torch_ops.sgm2d(Cv, r, r, P1, P2, layout="dhw", arith="exact")}
            if r == 4:
                Cs = Cv % 25
                calls["rows"] = lambda: torch_ops.sgm2d(Cs, r, r, 6, 32, layout="dhw", cost_bound=24)
            names = {}
            for k, call in calls.items():
                call()                                           # warm: plan, buffers
                names[k] = last_kernel()
                timed(call, 2)
            ms = {k: [] for k in calls}
            for _ in range(a.rounds):
                for k in ms:
                    ms[k].append(timed(calls[k], a.iters))
            mmm = {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in ms.items()}
            out = {"window": [2 * r + 1, 2 * r + 1], "frames": n, "kernels": names, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "min_median_max": mmm, "exact_over_wrap": round(mmm["exact"][1] / mmm["wrap"][1], 3)}
            if "rows" in mmm:
                out["exact_over_rows"] = round(mmm["exact"][1] / mmm["rows"][1], 3)
            print(json.dumps(out), flush=True)
            del Cv
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
