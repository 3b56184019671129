"""Device time of sgm(C) with exact path arithmetic beside the plain (mod-256) call of the same build, warm, on one
1242x375x128 volume of random bytes, 8 paths, sgm.m's P1 = 7, P2 = 100: the case the exact mode exists for, where the plain
call runs "packed16/wrap".

For 1 and 8 frames, fsgm_sgm_device and fsgm_sgm_device_exact on the same tensors in HBM, interleaved in one process, each timed
by a pair of events on the caller's stream around `iters` back-to-back calls (ingest copy, line kernels, WTA).  The plain call
moves 24 B per voxel of line traffic (8 path volumes written, read once), the exact one 25 (the WTA reads C as well): the
expectation is exact <= 25/24 of the plain median plus the plain call's own min-to-max spread.  Every figure of every round is
printed (ms per call) and min / median / max per state at the end, as JSON lines.

    python3 tools/sgm_exact_timing.py [--rounds 7] [--iters 20] [--batches 1,8]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # noqa: I001 -- first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsgm_amd import torch_ops  # noqa: E402
from fsgm_amd.sgm import last_kernel  # noqa: E402

W, H, D, PATHS, P1, P2 = 1242, 375, 128, 8, 7, 100


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    print(json.dumps({"shape": [W, H, D], "paths": PATHS, "P1": P1, "P2": P2, "costs": "uniform random bytes", "iters": a.iters,
                      "rounds": a.rounds}))
    g = torch.Generator(device="cuda").manual_seed(3)
    for n in [int(b) for b in a.batches.split(",")]:
        Cv = torch.randint(0, 256, (n, H, W, D), dtype=torch.uint8, device="cuda", generator=g)
        calls, names = {}, {}
        for arith in ("mod256", "exact"):
            calls[arith] = lambda arith=arith: torch_ops.sgm(Cv, P1, P2, layout="hwd", paths=PATHS, arith=arith)
            calls[arith]()                                       # warm: plan, buffers
            names[arith] = last_kernel()
            timed(calls[arith], 3)
        ms = {"mod256": [], "exact": []}
        for _ in range(a.rounds):
            for arith in ms:
                ms[arith].append(timed(calls[arith], a.iters))
        mmm = {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in ms.items()}
        plain = mmm["mod256"]
        bound = plain[1] * 25.0 / 24.0 + (plain[2] - plain[0])
        print(json.dumps({"frames": n, "kernels": names, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                          "min_median_max": mmm, "exact_over_mod256": round(mmm["exact"][1] / plain[1], 3),
                          "expected_at_most_ms": round(bound, 4), "within": bool(mmm["exact"][1] <= bound)}), flush=True)
        del Cv
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
