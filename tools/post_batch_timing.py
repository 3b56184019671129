"""Device time per 1242x375 map of the post-processing chain (test.m:45-50) on batches, and of test.m's whole frame body
(fsgm_amd.torch_ops.epipolar_flow_pp) beside epipolar_sgm_of, warm, from events on the caller's stream.  Prints one JSON line.

  chain_ms_per_map[N]        torch_ops.epi_postprocess on N maps, median of `iters` calls, divided by N (N = 1, 8, 32)
  chain_plan_ms              the single-map PostPlan's own back-to-back time (fsgm_post_plan_time), the earlier figure
  flow_pp_ms_per_frame[N]    torch_ops.epipolar_flow_pp on N pairs (dMax 64, 4 paths), per frame (N = 1, 8)
  sgm_of_ms_per_frame[N]     torch_ops.epipolar_sgm_of on the same pairs, per frame
  oracle_ms_per_map          the CPU oracle's chain on one map (oracle.postprocess), median of 3

    python3 tools/post_batch_timing.py [--iters 10]
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
from fsgm_amd import torch_ops, synth  # noqa: E402

DEV = "cuda:0"
W, H, D, VMAX = 1242, 375, 64, 0.3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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


def maps(N):
    D1 = np.stack([synth.vz_index_map(W, H, D, seed=f) for f in range(N)])
    p, n, o = synth.epi_maps(W, H, "general", seed=2)
    rep = lambda a: np.broadcast_to(a, (N,) + a.shape).copy()  # noqa: E731
    return D1, rep(p), rep(n), rep(o / 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    out = {"shape": [W, H], "dMax": D, "iters": a.iters, "chain_ms_per_map": {}, "flow_pp_ms_per_frame": {}, "sgm_of_ms_per_frame": {}}
    for N in (1, 8, 32):
        args = [_t(x) for x in maps(N)]
        out["chain_ms_per_map"][N] = device_ms(lambda: torch_ops.epi_postprocess(*args, VMAX, D + 1, D), a.iters) / N
        del args
        torch.cuda.empty_cache()
    m = maps(1)
    with fsgm_amd.PostPlan(W, H) as plan:
        plan.upload(m[0][0], m[1][0], m[2][0], m[3][0])
        out["chain_plan_ms"] = plan.time(VMAX, D + 1, D, warmup=2, iters=a.iters)
    for N in (1, 8):
        pairs = [synth.image_pair(W, H, 12, seed=10 + f) for f in range(N)]
        geos = [synth.epi_geometry(W, H, "forward" if f % 2 == 0 else "contract") for f in range(N)]
        I0, I1 = _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))
        F, Hm, e, d = (list(x) for x in zip(*geos))
        out["flow_pp_ms_per_frame"][N] = device_ms(lambda: torch_ops.epipolar_flow_pp(I0, I1, F, Hm, e, d, D, VMAX), a.iters) / N
        out["sgm_of_ms_per_frame"][N] = device_ms(lambda: torch_ops.epipolar_sgm_of(I0, I1, F, Hm, e, d, D, VMAX), a.iters) / N
    from oracle import pyoracle
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        pyoracle.postprocess(m[0][0], m[1][0], m[2][0], m[3][0], VMAX, D + 1, D)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["oracle_ms_per_map"] = statistics.median(ts)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
