"""Device time of the quantising float ingest (fsgm_epi_plan_ingest_float_dptr / fsgm_pyd_plan_ingest_float_dptr) beside what a
caller had to run without it, at 1242x375x128 (N, D, H, W) for the 1-D matcher and at a 9x9 window (N, 81, H, W) for the 2-D
matcher, N = 1 and 8; warm, from events on the caller's stream, the variants of one shape taken in turn inside every round so that
they share the machine's noise.  Prints one JSON line per shape.

  u8_ms             the u8 ingest of the same shape (ingest_cost / ingest_cost2d): median [min, max] over the rounds -- its spread
                    is the yardstick for every ratio below
  float_ms[dtype]   the float ingest of a float32 / float16 / bfloat16 tensor of that shape: median [min, max]
  torch_ms[dtype]   (c * s + o).round().clamp(0, b).to(torch.uint8) on the same tensor: four elementwise passes and three
                    temporaries; its result still has to go through the u8 ingest
  ratio[dtype]      float_ms / u8_ms, beside bytes_ratio = (element size + 1) / 2: what the byte counts alone predict
  gbps[dtype]       source bytes read + one byte a voxel written, over float_ms (the 2-D plan's padding bytes are not counted)

    python3 tools/sgm_float_ingest_timing.py [--rounds 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: the library binds to torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsgm_amd import torch_ops, EpiPlan, PydPlan  # noqa: E402

DEV = "cuda:0"
W, H, D1, HALF, BOUND, SCALE, OFFSET = 1242, 375, 128, 4, 24, 0.1, 0.25
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def timed(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(times):
    return [statistics.median(times), min(times), max(times)]


def measure(family, n, rounds):
    D = D1 if family == "sgm" else (2 * HALF + 1) ** 2
    plan = EpiPlan(W, H, D, n, vz_to_disp=0) if family == "sgm" else PydPlan(W, H, W, H, HALF, HALF, 0, batch=n)
    ingest_u8 = torch_ops.ingest_cost if family == "sgm" else torch_ops.ingest_cost2d
    ingest_f = torch_ops.ingest_cost_float if family == "sgm" else torch_ops.ingest_cost2d_float
    with plan:
        u8 = torch.randint(0, BOUND + 1, (n, D, H, W), dtype=torch.uint8, device=DEV)
        floats = {name: ((u8.float() - OFFSET) / SCALE).to(dt) for name, dt in DTYPES.items()}
        variants = {"u8": lambda: ingest_u8(plan, u8, layout="dhw", cost_bound=BOUND)}
        for name, t in floats.items():
            variants["float/" + name] = lambda t=t: ingest_f(plan, t, SCALE, OFFSET, layout="dhw", cost_bound=BOUND)
            variants["torch/" + name] = lambda t=t: (t * SCALE + OFFSET).round().clamp(0, BOUND).to(torch.uint8)
        times = {k: [] for k in variants}
        for r in range(-2, rounds):                               # two warm rounds
            for k, fn in variants.items():
                ms = timed(fn)
                if r >= 0:
                    times[k].append(ms)
        # what was timed computes the torch expression's bytes (no tie among these values, and torch runs the multiply and the add apart)
        st = ingest_f(plan, floats["float32"], SCALE, OFFSET, layout="dhw", cost_bound=BOUND, return_status=True)
        want = (floats["float32"] * SCALE + OFFSET).round().clamp(0, BOUND).to(torch.uint8)
        assert int(st.item()) == 0
        got = torch.from_numpy(plan.download_cost(n - 1)).to(DEV)
        assert torch.equal(got, want[n - 1].permute(1, 2, 0)), "the timed ingest does not compute the torch expression's bytes"
    voxels = n * D * H * W
    u8_med = statistics.median(times["u8"])
    out = {"family": family, "shape": [n, D, H, W], "rounds": rounds, "cost_bound": BOUND, "u8_ms": summary(times["u8"]),
           "float_ms": {}, "torch_ms": {}, "ratio": {}, "bytes_ratio": {}, "gbps": {}}
    for name, dt in DTYPES.items():
        es = torch.empty((), dtype=dt).element_size()
        f = summary(times["float/" + name])
        out["float_ms"][name], out["torch_ms"][name] = f, summary(times["torch/" + name])
        out["ratio"][name], out["bytes_ratio"][name] = f[0] / u8_med, (es + 1) / 2
        out["gbps"][name] = voxels * (es + 1) / f[0] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fall-back")
    for family in ("sgm", "sgm2d"):
        for n in (1, 8):
            print(json.dumps(measure(family, n, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
