"""Device time of stereo_sgm_pp at 1242x375x128, warm, at N = 1 and 8.  Prints one JSON line.

  call_ms[N]            torch_ops.stereo_sgm_pp on N pairs in HBM: the whole call, median of events on the caller's stream
  matcher_call_ms[N]    torch_ops.stereo_sgm(d_min=0) on the same pairs, the same way: the matcher alone
  chain_ms[N]           call_ms - matcher_call_ms
  parts_ms[N]           fsgm_stereo_sgm_pp_time: events on the plan's stream around back-to-back runs of
                          matcher   the matcher alone
                          chain     the chain alone (index map, speckle filter, row kernel, island removal, in-fill, pack)
                          row       the fused row kernel alone (second-view map + check, LDS row)
                          generic   launch_disp_from_first + launch_fb_check of the epipolar chain on the same map with explicit
                                    rectified maps (Pd0, normDir, O = 1): 64-bit global atomics and three f64 map planes per pixel.
                                    Their disparity function is vzInd2Disp, not d_min + w: a cost comparison only
                        --repeats values each; their spread is the run-to-run noise of the session
  per_map_ms[N]         medians of parts_ms divided by N

    python3 tools/stereo_pp_timing.py [--iters 20] [--batches 1,8] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from fsgm_amd import stereo_pp, torch_ops, synth  # noqa: E402

DEV = "cuda:0"
W, H, D = 1242, 375, 128
PARTS = ("matcher", "chain", "row", "generic")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    base = [synth.image_pair(W, H, D, seed=s) for s in range(1, 5)]
    out = {"shape": [W, H, D], "iters": a.iters, "paths": 4, "call_ms": {}, "matcher_call_ms": {}, "chain_ms": {}, "parts_ms": {},
           "per_map_ms": {}}
    for n in (int(b) for b in a.batches.split(",")):
        pairs = [tuple(np.roll(x, 7 * (f // len(base)), axis=1) for x in base[f % len(base)]) for f in range(n)]
        L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        tL, tR = torch.from_numpy(L).to(DEV), torch.from_numpy(R).to(DEV)
        out["call_ms"][n] = device_ms(lambda: torch_ops.stereo_sgm_pp(tL, tR, D), a.iters)
        out["matcher_call_ms"][n] = device_ms(lambda: torch_ops.stereo_sgm(tL, tR, D, d_min=0), a.iters)
        out["chain_ms"][n] = out["call_ms"][n] - out["matcher_call_ms"][n]
        runs = [stereo_pp.stereo_sgm_pp_time(L, R, D, warmup=3, iters=a.iters) for _ in range(a.repeats)]
        out["parts_ms"][n] = {k: [r[i] for r in runs] for i, k in enumerate(PARTS)}
        out["per_map_ms"][n] = {k: statistics.median(v) / n for k, v in out["parts_ms"][n].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
