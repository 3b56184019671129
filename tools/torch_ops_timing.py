"""Warm per-call times of the device-pointer entry points (fsgm_amd.torch_ops) against the host entry points and the plans' own
device time for the same work.  Prints one JSON line per case.

  device_ms   median over `iters` calls of the time between two events recorded on the caller's stream around one call
  enqueue_ms  median host time of the call itself (it must return before the device is done: no host wait)
  host_ms     median wall time of the matching host entry point (numpy in, numpy out)
  plan_ms     fsgm_epi_plan_time / fsgm_pyramid_plan_time of the same work (kernels only, back to back)

    python3 tools/torch_ops_timing.py [--iters 20]
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
from fsgm_amd._lib import STAGE_ALL  # noqa: E402

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_times(fn, iters):
    s = torch.cuda.current_stream()
    fn()
    s.synchronize()
    evs, enq = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t = time.perf_counter()
        fn()
        enq.append((time.perf_counter() - t) * 1e3)
        e1.record(s)
        evs.append((e0, e1))
        s.synchronize()                      # one call at a time: the events time that call alone
    return statistics.median(a.elapsed_time(b) for a, b in evs), statistics.median(enq)


def host_time(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def rgb_pair(W, H, seed):
    I0, I1 = synth.image_pair(W, H, 12, seed=seed)
    return np.stack([I0, I0 // 2 + 60, 255 - I0]), np.stack([I1, I1 // 2 + 60, 255 - I1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    it = a.iters
    W, H = 1242, 375
    rows = []
    for D, paths, n in ((128, 4, 1), (128, 8, 1), (128, 4, 8), (128, 8, 8)):
        frames = []
        for f in range(n):
            I1, I2 = synth.image_pair(W, H, D, seed=1 + f)
            frames.append((I1, I2) + tuple(synth.epi_maps(W, H, "general", seed=7 + f)))
        dv = [_t(np.stack([fr[k] for fr in frames])) for k in range(5)]
        dev_ms, enq_ms = device_times(lambda: torch_ops.calc_cost_sgm(dv[0], dv[1], D, 0.3, dv[2], dv[3], dv[4], 6, 64, paths=paths), it)
        host_ms = host_time(lambda: fsgm_amd.calc_cost_sgm_batch(frames, D, 0.3, 6, 64, paths=paths), it)
        with fsgm_amd.EpiPlan(W, H, D, n, paths=paths) as plan:
            plan.set_penalties(6, 64, 0.3)
            for f, fr in enumerate(frames):
                plan.upload(f, *fr)
            plan_ms = plan.time(STAGE_ALL, warmup=2, iters=it)
        rows.append(dict(case=f"calc_cost_sgm {W}x{H}x{D} paths={paths} frames={n}", device_ms=dev_ms, enqueue_ms=enq_ms,
                         host_ms=host_ms, plan_ms=plan_ms))
    D = 64
    I0, I1 = synth.image_pair(W, H, 12, seed=5)
    g = synth.epi_geometry(W, H, "forward")
    d0, d1 = _t(I0), _t(I1)
    dev_ms, enq_ms = device_times(lambda: torch_ops.epipolar_sgm_of(d0, d1, *g, D, 0.3), it)
    host_ms = host_time(lambda: fsgm_amd.epipolar_sgm_of(I0, I1, *g, D, 0.3), it)
    Pd0, nd, off, _ = fsgm_amd.epipolar_maps(*g, W, H)
    with fsgm_amd.EpiPlan(W, H, D, 1) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload(0, I0, I1, Pd0, nd, off)
        plan_ms = plan.time(STAGE_ALL, warmup=2, iters=it)
    rows.append(dict(case=f"epipolar_sgm_of {W}x{H} D={D} gray", device_ms=dev_ms, enqueue_ms=enq_ms, host_ms=host_ms,
                     plan_ms=plan_ms, plan_note="cost+aggregation+WTA only (no maps, no flow)"))
    for ng in (False, True):
        host_fn = fsgm_amd.pyramidal_sgm_ng if ng else fsgm_amd.pyramidal_sgm
        dev_fn = torch_ops.pyramidal_sgm_ng if ng else torch_ops.pyramidal_sgm
        Plan = fsgm_amd.NgPyramidPlan if ng else fsgm_amd.PyramidPlan
        for n in (1, 8):
            pairs = [rgb_pair(W, H, 20 + f) for f in range(n)]
            a0, a1 = _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))
            dev_ms, enq_ms = device_times(lambda: dev_fn(a0, a1, 3, batch=True), it)
            host_ms = host_time(lambda: [host_fn(p[0], p[1], 3) for p in pairs], max(3, it // 4))
            with Plan(W, H, 3, 3, batch=n) as plan:
                for f, p in enumerate(pairs):
                    plan.upload(p[0], p[1], frame=f)
                plan_ms = plan.time(warmup=2, iters=it)
            rows.append(dict(case=f"pyramidal_sgm{'_ng' if ng else ''} {W}x{H} RGB 3 levels pairs={n}", device_ms=dev_ms,
                             enqueue_ms=enq_ms, host_ms=host_ms, plan_ms=plan_ms,
                             host_note="one host call per pair" if n > 1 else ""))
    for r in rows:
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)


if __name__ == "__main__":
    main()
