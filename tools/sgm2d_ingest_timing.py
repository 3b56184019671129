"""Device time of bringing 8 caller-supplied 2-D cost volumes of 1242x375x121 (an 11x11 window) into a plan's padded rows, in
each source layout, beside a device-to-device hipMemcpyAsync of the same byte count and the aggregation + WTA that follows;
warm, from events on the caller's stream.  Prints one JSON line.

  ingest_ms[layout]      PydPlan.ingest_cost (fsgm_pyd_plan_ingest_cost_device) of the 8 volumes, median of `iters` calls
                         (cost_bound 24: the saturating kernels, what a caller of the non-wrapping aggregation runs)
  ingest_gbps[layout]    source bytes read + padded bytes written, over that time
  copy_ms, copy_gbps     hipMemcpyAsync device to device of the source's byte count (read + written bytes counted)
  aggregate_wta_ms       the plan's own back-to-back time of aggregation + WTA on the ingested volumes (fsgm_pyd_plan_time;
                         P1 6, P2 32, 8 paths, 2 passes, zero hints)

    python3 tools/sgm2d_ingest_timing.py [--iters 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch  # first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from fsgm_amd import torch_ops, synth, PydPlan  # noqa: E402
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA  # noqa: E402

DEV = "cuda:0"
W, H, HALF, N, BOUND = 1242, 375, 5, 8, 24
SX = SY = 2 * HALF + 1
D = SX * SY


def device_ms(fn, iters):
    s = torch.cuda.current_stream()
    for _ in range(2):
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fall-back")
    hip = C.CDLL(torch_ops.hip_runtimes()[0])
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    one = synth.cost_volume(W, H, D, seed=3, cmax=BOUND)                          # (H, W, D), reference order
    src_bytes, dst_bytes = N * one.size, N * W * H * SX * 4 * ((SY + 3) // 4)
    out = {"shape": [W, H, D], "frames": N, "iters": a.iters, "cost_bound": BOUND, "src_bytes": src_bytes, "padded_bytes": dst_bytes,
           "ingest_ms": {}, "ingest_gbps": {}}
    with PydPlan(W, H, W, H, HALF, HALF, 0, batch=N) as plan:
        plan.set_params(6, 32, 1, 2, 0, 1)
        img, mv = np.zeros((H, W), np.uint8), np.zeros((2, H, W))
        for f in range(N):
            plan.upload(f, img, img, mv)
        forms = {"hwd": one, "dhw": one.transpose(2, 0, 1), "dhw_yx": one.reshape(H, W, SX, SY).transpose(3, 2, 0, 1).reshape(D, H, W)}
        for layout, v in forms.items():
            t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV).unsqueeze(0).repeat(N, 1, 1, 1).contiguous()
            ms = device_ms(lambda: plan.ingest_cost(t, layout=layout, cost_bound=BOUND), a.iters)
            out["ingest_ms"][layout] = ms
            out["ingest_gbps"][layout] = (src_bytes + dst_bytes) / ms / 1e6
            np.testing.assert_array_equal(plan.download_cost(N - 1), one)         # what was timed is the right transposition
            del t
        a_buf = torch.zeros(src_bytes, dtype=torch.uint8, device=DEV)
        b_buf = torch.empty(src_bytes, dtype=torch.uint8, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def copy():
            assert hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), src_bytes, 3, stream) == 0   # device to device
        out["copy_ms"] = device_ms(copy, a.iters)
        out["copy_gbps"] = 2 * src_bytes / out["copy_ms"] / 1e6
        out["aggregate_wta_ms"] = plan.time(STAGE_AGGREGATE | STAGE_WTA, warmup=2, iters=max(3, a.iters // 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
