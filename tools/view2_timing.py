"""Device time of the second view's kernel (epi_view2.hip) at 1242x375x128, 8 paths, batch 1 and 8, beside the line kernels' WTA of
the same plan and beside the torch formulation a caller would otherwise write on S.  Warm; the variants taken in turn inside every
round so that they share the machine's noise.  Prints one JSON line per batch.

  wta_ms        FSGM_STAGE_WTA of the plan with the switch off (EpiPlan.time): the WTA kernel alone, median [min, max] over the rounds
  wta_view2_ms  the same stage with the switch on: the WTA kernel and the second view's kernel behind it
  view2_ms      the difference of the two medians: the second view's kernel
  ratio         view2_ms / wta_ms, beside bytes_ratio = (T + D - 1) / T: the path-volume bytes the kernel reads over the WTA's one read
  torch_ms      on S int32 (N, H, W, D) in HBM (4 D bytes a pixel): gather along the diagonal, mask, argmin -- disp2 without sub-pixel

    python3 tools/view2_timing.py [--rounds 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsgm_amd import EpiPlan, synth, view2  # noqa: E402
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA  # noqa: E402

DEV = "cuda:0"
W, H, D, PATHS = 1242, 375, 128, 8


def summary(times):
    return [statistics.median(times), min(times), max(times)]


def torch_view2(S, x, ok, i):
    diag = S[:, :, x, i]                                         # (N, H, W, D): S[y][x2 + i][i]
    diag = torch.where(ok, diag, 1 << 30)
    return diag.argmin(-1)


def timed(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(n, rounds):
    Cv = synth.cost_volume(W, H, D, seed=2, cmax=24)
    S = torch.randint(0, 8 * 88, (n, H, W, D), dtype=torch.int32, device=DEV)
    i = torch.arange(D, device=DEV)[None, :]
    x = torch.arange(W, device=DEV)[:, None] + i
    ok, x = x < W, x.clamp(max=W - 1)
    times = {"wta": [], "wta_view2": [], "torch": []}
    with EpiPlan(W, H, D, n, paths=PATHS, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload_cost(0, Cv)
        for f in range(1, n):
            plan.copy_cost(f, 0, 17 * f)
        plan.set_agg_mode(1)                                     # the line kernels, as a plan with the switch on runs them
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        plan.sync()
        kernel = plan.kernel_name
        for r in range(-2, rounds):                              # two warm rounds
            plan.set_view2(0)
            a = plan.time(STAGE_WTA, 2, 10)
            plan.set_view2(1, -1)
            b = plan.time(STAGE_WTA, 2, 10)
            t = timed(lambda: torch_view2(S, x, ok, i))
            if r >= 0:
                times["wta"].append(a); times["wta_view2"].append(b); times["torch"].append(t)
        assert plan.kernel_name == kernel
    wta, both = statistics.median(times["wta"]), statistics.median(times["wta_view2"])
    T = view2.tile(D)
    return {"shape": [n, H, W, D], "paths": PATHS, "kernel": kernel, "rounds": rounds, "tile": T, "wta_ms": summary(times["wta"]),
            "wta_view2_ms": summary(times["wta_view2"]), "view2_ms": both - wta, "ratio": (both - wta) / wta, "bytes_ratio": (T + D - 1) / T,
            "torch_ms": summary(times["torch"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fall-back")
    for n in (1, 8):
        print(json.dumps(measure(n, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
