"""Device time of sgm(C) on cost volumes that are already in HBM, at 1242x375x128, warm.  Prints one JSON line and writes it to
profiles/sgm_device_timing.txt.

  ingest[layout]        the ingest kernel alone (EpiPlan.ingest_cost, --ingest-frames volumes): ms of each repeat, events on the
                        caller's stream; gbps = read + written bytes over the median; ratio = gbps / copy_probe_gbps
  copy_probe_gbps       fsgm_measure_copy_bandwidth of the same byte count, in the same session: the yardstick
  sgm_ms_per_frame[N]   torch_ops.sgm (layout "dhw", cost_bound 24, 8 paths, P1 = 6, P2 = 32) on N volumes: ms of each repeat / N
  kernel[N]             the pipeline those calls ran (fsgm_sgm_last_kernel)
  host_ms_per_frame[N]  the same tensors the way the library offered before: per frame permute + .cpu(), fsgm_amd.sgm, results
                        back to the GPU; wall clock, over min(N, --host-frames) frames

    python3 tools/sgm_device_timing.py [--repeats 5] [--batches 1,8,40] [--ingest-frames 8] [--host-frames 4]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch  # first: the library binds to torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, synth, torch_ops  # noqa: E402
from fsgm_amd.epi import EpiPlan  # noqa: E402
from fsgm_amd.sgm import last_kernel  # noqa: E402

DEV = "cuda:0"
W, H, D = 1242, 375, 128
P1, P2, PATHS, BOUND = 6, 32, 8, 24


def event_ms(fn, repeats):
    s = torch.cuda.current_stream()
    fn()                                                         # warm: plan, buffers
    s.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def volumes(n):
    """(n, D, H, W) uint8 on the GPU: two draws, rolled along x so that every frame differs"""
    base = [torch.from_numpy(synth.cost_volume(W, H, D, seed, BOUND)).to(DEV).permute(2, 0, 1).contiguous() for seed in (3, 4)]
    return torch.stack([torch.roll(base[f % 2], 7 * (f // 2), dims=2) for f in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,8,40")
    ap.add_argument("--ingest-frames", type=int, default=8)
    ap.add_argument("--host-frames", type=int, default=4)
    a = ap.parse_args()
    lib = _lib.load()
    out = {"shape": [W, H, D], "repeats": a.repeats, "paths": PATHS, "penalties": [P1, P2], "cost_bound": BOUND, "ingest": {},
           "sgm_ms_per_frame": {}, "kernel": {}, "host_ms_per_frame": {}}

    n = a.ingest_frames
    nbytes = n * W * H * D
    dhw = volumes(n)
    hwd = dhw.permute(0, 2, 3, 1).contiguous()
    gbps = C.c_double()
    _lib.check(lib.fsgm_measure_copy_bandwidth(0, nbytes, 10, C.byref(gbps)))
    out["copy_probe_gbps"] = gbps.value
    with EpiPlan(W, H, D, n, paths=PATHS, vz_to_disp=0) as plan:
        for layout, t in (("hwd", hwd), ("dhw", dhw)):
            for bound in (255, BOUND):                           # 255: nothing to saturate, the kernel skips the compare
                ms = event_ms(lambda: plan.ingest_cost(t, layout=layout, cost_bound=bound), a.repeats)
                rate = 2.0 * nbytes / (statistics.median(ms) * 1e-3) / 1e9
                out["ingest"][f"{layout}/bound{bound}"] = {"ms": ms, "gbps": rate, "ratio": rate / gbps.value}
    del hwd

    for n in (int(b) for b in a.batches.split(",")):
        t = dhw[:n] if n <= dhw.shape[0] else volumes(n)
        ms = event_ms(lambda: torch_ops.sgm(t, P1, P2, layout="dhw", paths=PATHS, cost_bound=BOUND), a.repeats)
        out["sgm_ms_per_frame"][n] = [m / n for m in ms]
        out["kernel"][n] = last_kernel()
        k = min(n, a.host_frames)

        def host():
            for f in range(k):
                Cv = t[f].permute(1, 2, 0).contiguous().cpu().numpy()
                bestD, minC = fsgm_amd.sgm(Cv, P1, P2, paths=PATHS)
                torch.from_numpy(bestD).to(DEV), torch.from_numpy(minC).to(DEV)
            torch.cuda.synchronize()
        host()
        walls = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            host()
            walls.append((time.perf_counter() - t0) * 1e3 / k)
        out["host_ms_per_frame"][n] = walls
        del t

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sgm_device_timing.txt"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
