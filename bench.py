#!/usr/bin/env python3
"""bench.py -- headline benchmark: aggregated cost-volume voxel-paths/s on synthetic KITTI-shape
volumes (1242 x 375 x 128, 8 paths), one process per GPU.

A "step" is one pass of the aggregation stage (multi-path DP over C, then sum + WTA + sub-pixel)
over one batch of --frames-per-gpu (default 512) cost volumes that are already resident in HBM.  Frames shard
across ranks with no collective in the data path (weak scaling: per-GPU batch fixed).

  python bench.py --gpus 1 --steps 20 --warmup 3
  python bench.py --gpus 1 --steps 20 --warmup 3 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the result line (metric, value,
ms_per_step, the configuration it ran).  Everything else the benchmark measures or checks takes runs of its own and is
behind --full: the self-check of the timed output against the line kernels, the stage times and the roofline block
(copy-bandwidth probes included), the whole-MEX and host-call legs and the CPU baselines.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, D, PATHS = 1242, 375, 128, 8
P1, P2, VMAX = 6, 64, 0.3
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# HBM/fabric bytes per voxel of the aggregation stage come from the newest rocprofv3 PMC summary under profiles/
# (tools/pmc_traffic.sh: FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for wide coalesced reads on gfx950,
# + WRITE_SIZE; separate passes).  The summary names the kernels it measured; a summary whose kernel set is not the
# one this build launches is not used (traffic = null).
def measured_traffic(kernel_name, paths):
    """bytes per voxel of the newest profiles/rNN_pmc_traffic*.json that measured this pipeline at this path count."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), reverse=True):
        try:
            t = json.load(open(f))
            if t.get("pipeline") == kernel_name and t.get("paths") == paths:
                return float(t["bytes_per_voxel"]), {"file": os.path.relpath(f, ROOT), "measured": t.get("date"), "head": t.get("head"), "lib_sha16": t.get("lib_sha16")}
        except Exception:
            pass
    return None, None


def lib_sha16():
    """sha256 (first 16 hex digits) of the library this run loads: the PMC summaries carry the same field, so a traffic figure
    measured on another build of the kernels shows (roofline.traffic_stale)."""
    import hashlib
    from fsgm_amd import _lib
    try:
        return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    except Exception:
        return None


DUMP_BYTES_MAX = 64 * 10**6


def dump_outputs(dirpath, plan, B):
    """--dump-outputs DIR: what the timed plan's last step left for a caller of EpiPlan.download (bestD, minC; u32 [H][W]
    per frame) on a fixed sample of frames spread over the batch (first and last included), as float64 (exact for u32)
    stacked [frames][H][W]: DIR/bestD.npy, DIR/minC.npy.  As many frames as fit in DUMP_BYTES_MAX, at most 8."""
    import numpy as np
    n = max(1, min(8, B, DUMP_BYTES_MAX // (2 * 8 * W * H)))
    frames = sorted({int(round(i * (B - 1) / (n - 1))) for i in range(n)}) if n > 1 else [0]
    got = [plan.download(f) for f in frames]
    os.makedirs(dirpath, exist_ok=True)
    files = {}
    for k, name in enumerate(("bestD", "minC")):
        a = np.stack([g[k] for g in got]).astype(np.float64)
        np.save(os.path.join(dirpath, name + ".npy"), a)
        files[name] = list(a.shape)
    return {"dir": dirpath, "frames": frames, "dtype": "float64", "files": files}


def cpu_baseline(sample_rows=48, PATHS=PATHS):
    """The CPU oracle (a port: oracle/fsgm_oracle_epi.cpp, 1 thread like the reference) timed on a
    bounded sample of the same workload: 8-path aggregation of a 1242 x sample_rows x 128 strip."""
    import numpy as np
    from fsgm_amd import synth
    from oracle import pyoracle
    Cv = synth.cost_volume(W, sample_rows, D, seed=5, cmax=24)
    pyoracle.epi_aggregate(Cv[:8], P1, P2, PATHS)          # warm up / page in
    t0 = time.perf_counter()
    reps = 0
    while True:
        pyoracle.epi_aggregate(Cv, P1, P2, PATHS)
        reps += 1
        dt = time.perf_counter() - t0
        if dt > 10.0 or reps >= 120:
            break
    vp = reps * W * sample_rows * D * PATHS
    return {"value": vp / dt, "unit": "voxel-paths/s", "cores": 1, "kind": "port",
            "sample": f"oracle fsgm_oracle_epi_aggregate, {reps} x (1242x{sample_rows}x128, {PATHS} paths), {dt:.1f} s"}


def cpu_baseline_all_cores(sample_rows=48, PATHS=PATHS, seconds=8.0):
    """The same oracle on every host core the process may use, one independent strip per thread (frames
    and strips are independent: the only parallelism a CPU port gets without changing the algorithm).
    SURVEY 8(d) asks for it beside the single-threaded figure; it is not the reference's configuration."""
    import os
    import threading
    from fsgm_amd import synth
    from oracle import pyoracle
    T = max(1, min(len(os.sched_getaffinity(0)), 16))                  # the box's CPU share for one GPU
    vols = [synth.cost_volume(W, sample_rows, D, seed=5 + t, cmax=24) for t in range(T)]
    reps = [0] * T
    t0 = time.perf_counter()

    def work(t):
        while time.perf_counter() - t0 < seconds:
            pyoracle.epi_aggregate(vols[t], P1, P2, PATHS)      # ctypes call: releases the GIL
            reps[t] += 1

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    return {"value": sum(reps) * W * sample_rows * D * PATHS / dt, "unit": "voxel-paths/s", "cores": T, "kind": "port",
            "sample": f"{T} threads x oracle fsgm_oracle_epi_aggregate on 1242x{sample_rows}x128 strips, {sum(reps)} strips, {dt:.1f} s"}


def pyramid3(args):
    """BASELINE config 4: pyramidal 2-D path, 1242x375 RGB pair, 3-level pyramid (test_psgm.m:33), 11x11 window,
    8 paths, 2 passes, P1=6, P2=32 (pyramidal_sgm.m:15-22).  value = milliseconds of one whole
    pyramidal_sgm on the device (image pyramid, rgb2gray, three calc_pyd_cost_sgm levels, flow
    composition; HIP events on the plan's stream); per-level stage times and the host-pointer call
    (PCIe-inclusive) are reported beside it."""
    import numpy as np
    import fsgm_amd
    from fsgm_amd import synth, PydPlan, PyramidPlan, pyramidal_sgm
    from fsgm_amd._lib import STAGE_COST, STAGE_AGGREGATE, STAGE_WTA
    iters = max(3, args.steps // 4)
    g0, g1 = synth.image_pair(W, H, 16, seed=2)
    I0 = np.stack([g0, 255 - g0, g0 // 2 + 40])
    I1 = np.stack([g1, 255 - g1, g1 // 2 + 40])
    with PyramidPlan(W, H, 3, 3) as plan:
        plan.upload(I0, I1)
        total = plan.time(2, iters)
        sizes = [plan.level_size(l) for l in (3, 2, 1)]
    # the drop-in call (host pointers in and out, PCIe included): with freshly allocated outputs every call, as the Python
    # wrapper makes them, and with the outputs of the previous call handed back (resident pages: what a MEX gateway's
    # zero-filled plhs arrays are to the library)
    res = pyramidal_sgm(I0, I1, 3)                            # builds the cached plan
    for _ in range(3):
        pyramidal_sgm(I0, I1, 3)
    hn = max(10, iters)
    t0 = time.perf_counter()
    for _ in range(hn):
        pyramidal_sgm(I0, I1, 3)
    host_ms = (time.perf_counter() - t0) / hn * 1e3
    t0 = time.perf_counter()
    for _ in range(hn):
        pyramidal_sgm(I0, I1, 3, out=res)
    host_reuse_ms = (time.perf_counter() - t0) / hn * 1e3
    # throughput form: independent plans (one stream each) started before any is waited for
    in_flight = {}
    for n in (2, 4, 8):
        plans = [PyramidPlan(W, H, 3, 3) for _ in range(n)]
        try:
            for f, pl in enumerate(plans):
                pl.upload(np.roll(I0, 13 * f, axis=2), np.roll(I1, 13 * f, axis=2))
            rounds = max(3, iters)
            for timed in (False, True):
                t0 = time.perf_counter()
                for _ in range(rounds):
                    for pl in plans:
                        pl.run()
                for pl in plans:
                    pl.sync()
                dt = time.perf_counter() - t0
            in_flight[str(n)] = {"ms_per_pair": dt / (rounds * n) * 1e3, "pairs_per_s": rounds * n / dt, "speedup_vs_sequential": total * rounds * n / (dt * 1e3)}
        finally:
            for pl in plans:
                pl.close()
    # a batch of pairs resident in one plan: every kernel of a level covers all of them
    batched = {}
    for Bn in (4, 8, 16):
        with PyramidPlan(W, H, 3, 3, batch=Bn) as plan:
            for f in range(Bn):
                plan.upload(np.roll(I0, 13 * f, axis=2), np.roll(I1, 13 * f, axis=2), frame=f)
            ms = plan.time(1, max(2, iters // 2))
        batched[str(Bn)] = {"ms_per_batch": ms, "ms_per_pair": ms / Bn, "pairs_per_s": Bn / (ms * 1e-3), "speedup_vs_sequential": total * Bn / ms}
    levels = []
    for (w, h) in sizes:                                      # coarse to fine, stage by stage
        with PydPlan(w, h, w, h, 5, 5, 2, 1) as lp:
            lp.set_params(6, 32, 1, 2, 0, int((w, h) == (W, H)))
            a, b = synth.image_pair(w, h, 16, seed=2)
            lp.upload(0, a, b, synth.hint_map(w, h, "even", seed=3))
            ms = [lp.time(st, 1, iters) for st in (STAGE_COST, STAGE_AGGREGATE, STAGE_WTA)]
        levels.append({"size": [w, h], "cost_ms": ms[0], "aggregate_ms": ms[1], "wta_ms": ms[2]})
    vp = sum(w * h for (w, h) in sizes) * 121 * 8
    print(json.dumps({"metric": "pyramidal_sgm (3-level calc_pyd_cost_sgm pyramid), device time per image pair", "value": total, "unit": "ms",
                      "higher_is_better": False, "n_gpus": 1, "dtype": "u8", "data": "synthetic",
                      "config": {"workload": "pyramid 1242x375 / 621x188 / 311x94 RGB, 11x11 window (D=121), 8 paths, 2 passes"},
                      "voxel_paths_per_s": vp / (total * 1e-3), "host_call_ms": host_ms, "host_call_outputs_reused_ms": host_reuse_ms,
                      "plans_in_flight": in_flight, "batched": batched, "levels": levels}), flush=True)


def pyramid3_ng(args):
    """BASELINE config 4 read literally ("calc_pyd_cost_sgm_ng ... 3-level pyramid"): the pyramidal level loop with the
    neighbour-guided MEX swapped in (fsgm_amd.pyramidal_sgm_ng / NgPyramidPlan; 81 candidates per pixel, 4 paths,
    2 passes, P1=6, P2=32 as ng_sgm.m:7-8,20).  value = milliseconds of one whole loop on the device (image pyramid,
    rgb2gray, three levels of census + candidate costs + aggregation + WTA, hint upsampling; HIP events on the
    plan's stream); the one-shot host call (plan creation and PCIe included) is reported beside it."""
    import numpy as np
    from fsgm_amd import synth, pyramidal_sgm_ng, NgPyramidPlan
    iters = max(3, args.steps // 4)
    g0, g1 = synth.image_pair(W, H, 16, seed=2)
    I0 = np.stack([g0, 255 - g0, g0 // 2 + 40])
    I1 = np.stack([g1, 255 - g1, g1 // 2 + 40])
    with NgPyramidPlan(W, H, 3, 3) as plan:
        plan.upload(I0, I1)
        total = plan.time(1, iters)
        sizes = [plan.level_size(l) for l in (3, 2, 1)]
    res = pyramidal_sgm_ng(I0, I1, 3)
    for _ in range(3):
        pyramidal_sgm_ng(I0, I1, 3)
    hn = max(10, iters)
    t0 = time.perf_counter()
    for _ in range(hn):
        pyramidal_sgm_ng(I0, I1, 3)
    host_ms = (time.perf_counter() - t0) / hn * 1e3
    t0 = time.perf_counter()
    for _ in range(hn):
        pyramidal_sgm_ng(I0, I1, 3, out=res)
    host_reuse_ms = (time.perf_counter() - t0) / hn * 1e3
    vp = sum(w * h for (w, h) in sizes) * 81 * 4
    # throughput form: a batch of pairs resident, every kernel of a level covers all of them
    batch = {}
    for Bn in (4, 8, 16):
        with NgPyramidPlan(W, H, 3, 3, batch=Bn) as plan:
            for f in range(Bn):
                plan.upload(np.roll(I0, 13 * f, axis=2), np.roll(I1, 13 * f, axis=2), frame=f)
            ms = plan.time(1, max(2, iters // 2))
        batch[str(Bn)] = {"ms_per_batch": ms, "ms_per_pair": ms / Bn, "pairs_per_s": Bn / (ms * 1e-3), "speedup_vs_sequential": total * Bn / ms}
    print(json.dumps({"metric": "pyramidal level loop with calc_pyd_cost_sgm_ng (3 levels), device time per image pair",
                      "value": total, "unit": "ms", "higher_is_better": False, "n_gpus": 1, "dtype": "u8", "data": "synthetic",
                      "config": {"workload": "pyramid 1242x375 / 621x188 / 311x94 RGB, 81 candidates per pixel, 4 paths, 2 passes"},
                      "voxel_paths_per_s": vp / (total * 1e-3), "host_call_ms": host_ms, "host_call_outputs_reused_ms": host_reuse_ms, "batched": batch}), flush=True)


def postprocess(args):
    """the post-processing chain of test.m:45-50 (speckle filter x2, calc_disp_from_first,
    forward-backward check, scan-line infill, vzInd2Disp) on a 1242x375 vz-index map, dMax = 64 (test.m:4).
    value = device milliseconds per map (HIP events); the CPU oracle's time for the same map beside it."""
    import numpy as np
    import fsgm_amd
    from fsgm_amd import synth, PostPlan, epi_postprocess
    from oracle import pyoracle
    D, vMax = 64, 0.3
    D1 = synth.vz_index_map(W, H, D, seed=8)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=2)
    off = off / 8
    iters = max(5, args.steps)
    with PostPlan(W, H) as plan:
        plan.upload(D1, pd0, nd, off)
        ms = plan.time(vMax, D + 1, D, 2, iters)
    epi_postprocess(D1, pd0, nd, off, vMax, D + 1, D)
    t0 = time.perf_counter()
    for _ in range(iters):
        epi_postprocess(D1, pd0, nd, off, vMax, D + 1, D)
    host_ms = (time.perf_counter() - t0) / iters * 1e3
    t0 = time.perf_counter()
    for _ in range(3):
        pyoracle.postprocess(D1, pd0, nd, off, vMax, D + 1, D)
    cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    print(json.dumps({"metric": "post-processing chain test.m:45-50, device time per 1242x375 map", "value": ms, "unit": "ms",
                      "higher_is_better": False, "n_gpus": 1, "dtype": "f64", "data": "synthetic",
                      "config": {"workload": "speckle_filter(2,100) + calc_disp_from_first + forward_backward_check + "
                                             "speckle_filter(64, rows*cols/10) + scanline_in_fill + vzInd2Disp, 1242x375"},
                      "pixels_per_s": W * H / (ms * 1e-3), "host_call_ms": host_ms,
                      "cpu_baseline": {"value": cpu_ms, "unit": "ms", "cores": 1, "kind": "port", "sample": "oracle fsgm_oracle_postprocess, same map, 3 runs"}}),
          flush=True)


def _pci_bus_id(dev):
    try:
        import ctypes as _C
        hip = _C.CDLL("libamdhip64.so")
        buf = _C.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(dev)) == 0:
            return buf.value.decode()
    except Exception:
        pass
    return str(dev)


def in_process(args):
    """--in-process N: the headline step on N devices from THIS process -- what a MATLAB session (one process) gets through the
    device lists of the C ABI (include/fsgm.h): one plan + stream per device-list entry, entry i on device i mod the device
    count, frames sharded by entry, no collective.  Weak scaling like the torchrun form: --frames-per-gpu frames per entry.
    On a one-GPU box every entry is device 0 (the entries then share the GPU: a rehearsal of the plumbing, not a scaling point)."""
    import numpy as np
    import fsgm_amd
    from fsgm_amd import synth, EpiPlan
    from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA
    PATHS = args.paths
    N = args.in_process
    ndev = fsgm_amd.load_library().fsgm_device_count()
    assert ndev >= 1, "bench.py needs a GPU"
    devs = [i % ndev for i in range(N)]
    B = args.frames_per_gpu
    _, _, off = synth.epi_maps(W, H, "axis")
    plans, check = [], []
    for slot, dev in enumerate(devs):
        plan = EpiPlan(W, H, D, B, paths=PATHS, device=dev)
        plan.set_penalties(P1, P2, VMAX)
        if args.agg_mode:
            plan.set_agg_mode(args.agg_mode)
        bases = [synth.cost_volume(W, H, D, seed=1000 * slot + s, cmax=24) for s in range(min(4, B))]
        for f in range(B):
            if f < 4:
                plan.upload_cost(f, bases[f])
            else:
                plan.copy_cost(f, f % 4, 37 * (f // 4))
            plan.upload_offset(f, off)
        plan.sync()
        check.append(bases[0])
        plans.append(plan)
    stages = STAGE_AGGREGATE | STAGE_WTA
    for _ in range(args.warmup):
        for pl in plans:
            pl.run(stages)
    for pl in plans:
        pl.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for pl in plans:                                    # asynchronous: every entry's step is queued before any is waited for
            pl.run(stages)
    for pl in plans:
        pl.sync()
    dt = time.perf_counter() - t0
    dumped = dump_outputs(args.dump_outputs, plans[0], B) if args.dump_outputs else None
    bus = [_pci_bus_id(d) for d in devs]
    vps = N * B * W * H * D * PATHS
    out = {"metric": f"aggregated cost-volume voxel-paths/s (HxWxDx{PATHS} paths), KITTI 1242x375 D=128", "value": vps * args.steps / dt,
           "unit": "voxel-paths/s", "n_gpus": len(set(bus)), "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
           "config": {"workload": f"KITTI 1242x375 D=128, {PATHS} paths, aggregation stage (C resident in HBM -> bestD/minC)",
                      "frames_per_gpu": B, "total_frames": N * B, "in_process_entries": N, "device_list": devs, "kernel": plans[0].kernel_name,
                      "sharding": "frames by device-list entry inside one process, no collective", "pci_bus_ids": bus, "distinct_devices": len(set(bus))},
           "full": bool(args.full), "argv": " ".join(sys.argv[1:])}
    if dumped:
        out["dump_outputs"] = dumped
    if args.full:
        # self-check: frame 0 of every entry against the line kernels on the same volume
        ok = True
        for slot, pl in enumerate(plans):
            got = pl.download(0)
            with EpiPlan(W, H, D, 1, paths=PATHS, device=devs[slot]) as ref:
                ref.set_penalties(P1, P2, VMAX)
                ref.set_agg_mode(1)
                ref.upload_cost(0, check[slot])
                ref.upload_offset(0, off)
                ref.run(stages)
                r = ref.download(0)
            ok = ok and np.array_equal(got[0], r[0]) and np.array_equal(got[1], r[1])
        assert ok, "an entry's bestD/minC differ from the line kernels' on the same volume"
        alg = B * W * H * D * PATHS
        stage_ms = plans[0].time(STAGE_AGGREGATE, warmup=1, iters=3)
        achieved = alg / (stage_ms * 1e-3) / 1e9
        out["roofline"] = {"bound": "hbm", "kernel": "aggregation stage of entry 0 alone", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes": alg, "stage_ms": stage_ms}
        out["checked"] = True
    for pl in plans:
        pl.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames-per-gpu", type=int, default=512,
                    help="frames resident per GPU and processed per step.  512 = one band-sweep workgroup per frame, two per CU "
                         "(31 GB of cost volumes, 118 GB with the plan's other buffers: what 288 GB of HBM are for); the block "
                         "sweeps' optimum is 40 (two lanes of 20), the line kernels take single frames")
    ap.add_argument("--total-frames", type=int, default=0,
                    help="strong scaling: a fixed batch of this many frames split over the ranks by fsgm_amd.batch.shard_indices "
                         "(BASELINE config 5 literally = 8); default 0 = weak scaling with --frames-per-gpu frames on every GPU")
    ap.add_argument("--agg-mode", type=int, default=0, choices=[0, 1, 2, 3, 4, 5, 6],
                    help="force an aggregation pipeline (fsgm_epi_plan_set_agg_mode): 0 auto (default), 1 line kernels, 2 fused sweeps / pairs, "
                         "3 parallel sweeps, 4 band sweeps, 5 chained band sweeps, 6 parallel sweeps meeting in the middle")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline figure does not need: the self-check of the timed output against "
                         "the line kernels (checked), the stage times and the roofline block, the whole-MEX and host-call legs, the CPU "
                         "baselines.  Off by default: a plain run sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baselines out")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: only the timed loop, the self-check and the roofline block (no whole-MEX / host-call legs): for profiler runs")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo to rehearse on one GPU)")
    ap.add_argument("--paths", type=int, default=8, choices=[4, 8],
                    help="8 = the headline metric (default); 4 = the reference's shipped configuration (no diagonal "
                         "paths, calc_cost_sgm.cpp:104) through the pair kernels -- secondary, not the judged line")
    ap.add_argument("--workload", default="epi8", choices=["epi8", "pyramid3", "pyramid3_ng", "postprocess"],
                    help="epi8 = the headline metric (default); pyramid3 = BASELINE config 4, one pyramidal_sgm at 1242x375 "
                         "(3 levels); postprocess = the test.m:45-50 chain on a 1242x375 map (both secondary, 1 GPU, "
                         "not the judged line)")
    ap.add_argument("--in-process", type=int, default=0,
                    help="N > 0: the headline step on N device-list entries from this one process (entry i on device i mod the device "
                         "count; what a single MATLAB process gets through the C ABI's device lists); prints the distinct PCI bus ids")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (bestD, minC of a fixed sample of frames, "
                         "float64) as DIR/<name>.npy, to compare two builds output for output (epi8 workload)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.in_process <= 0 and args.workload != "epi8":
        ap.error("--dump-outputs covers the epi8 workload (the headline step) only")
    if args.in_process > 0:
        return in_process(args)
    if args.workload == "pyramid3":
        return pyramid3(args)
    if args.workload == "pyramid3_ng":
        return pyramid3_ng(args)
    if args.workload == "postprocess":
        return postprocess(args)

    PATHS = args.paths
    import numpy as np
    import torch
    import torch.distributed as dist
    import fsgm_amd
    from fsgm_amd import synth, EpiPlan
    from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA, STAGE_COST

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    local_rank %= torch.cuda.device_count()                  # one process per GPU; wraps only when rehearsing on fewer GPUs
    torch.cuda.set_device(local_rank)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)

    # which physical devices the ranks sit on: the PCI bus ids, gathered to rank 0 (a real N-GPU run shows N distinct ids)
    bus_id = torch.cuda.get_device_properties(local_rank).pci_bus_id if hasattr(torch.cuda.get_device_properties(local_rank), "pci_bus_id") else -1
    try:
        import ctypes as _C
        _hip = _C.CDLL("libamdhip64.so")
        _buf = _C.create_string_buffer(64)
        if _hip.hipDeviceGetPCIBusId(_buf, 64, local_rank) == 0:
            bus_id = _buf.value.decode()
    except Exception:
        pass
    bus_ids = [str(bus_id)]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, str(bus_id))
        bus_ids = gathered

    from fsgm_amd.batch import shard_indices
    strong = args.total_frames > 0
    my_frames = shard_indices(args.total_frames, rank, world) if strong else list(range(args.frames_per_gpu))
    assert my_frames, f"rank {rank} of {world} gets no frame out of --total-frames {args.total_frames}"
    B = len(my_frames)
    plan = EpiPlan(W, H, D, B, paths=PATHS, device=local_rank)
    plan.set_penalties(P1, P2, VMAX)
    _, _, off = synth.epi_maps(W, H, "axis")
    # distinct volume per (rank, frame): 4 seeded base volumes per rank, the others are column
    # rotations of them (cheap to make, still all different)
    bases = [synth.cost_volume(W, H, D, seed=1000 * rank + s, cmax=24) for s in range(min(4, B))]

    def frame_volume(f):
        return bases[f] if f < 4 else np.ascontiguousarray(np.roll(bases[f % 4], 37 * (f // 4), axis=1))

    if args.agg_mode:
        plan.set_agg_mode(args.agg_mode)
    for f in range(B):
        if f < 4:
            plan.upload_cost(f, frame_volume(f))
        else:
            plan.copy_cost(f, f % 4, 37 * (f // 4))         # the same rotation, device to device (no PCIe transfer per frame)
        plan.upload_offset(f, off)
    plan.sync()
    if args.full:
        check_frames = sorted({int(round(i * (B - 1) / 15)) for i in range(16)}) if B > 1 else [0]     # 16 frames spread over the batch
        check_vols = [frame_volume(f) for f in check_frames]
    del bases
    stages = STAGE_AGGREGATE | STAGE_WTA

    def barrier():
        torch.cuda.synchronize()                             # the plan's own stream too (device-wide)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        plan.run(stages)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        plan.run(stages)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device="cuda" if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dumped = dump_outputs(args.dump_outputs, plan, B) if args.dump_outputs and rank == 0 else None

    def result_line():
        """What a plain run prints: the headline figure and the configuration it ran (nothing here launches a kernel)."""
        total_frames = args.total_frames if strong else world * B
        out = {
            "metric": f"aggregated cost-volume voxel-paths/s (HxWxDx{PATHS} paths), KITTI 1242x375 D=128",
            "value": total_frames * W * H * D * PATHS * args.steps / dt, "unit": "voxel-paths/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"KITTI 1242x375 D=128, {PATHS} paths, aggregation stage (C resident in HBM -> bestD/minC)",
                       "frames_per_gpu": B, "total_frames": total_frames, "P1": P1, "P2": P2, "kernel": plan.kernel_name,
                       "step": f"aggregate({PATHS} paths) + sum/WTA/subpixel", "sharding": "frames, no collective",
                       "pci_bus_ids": bus_ids, "distinct_devices": len(set(bus_ids))},
            "full": bool(args.full), "argv": " ".join(sys.argv[1:]),
        }
        if dumped:
            out["dump_outputs"] = dumped
        return out

    if not args.full:
        if rank == 0:
            print(json.dumps(result_line()), flush=True)
        plan.close()
        if world > 1:
            dist.destroy_process_group()
        return

    # --full from here on: checks and measurements beside the headline figure, each with runs of its own
    # self-check of what the timed loop left behind: two frames of the timed plan against the per-direction line
    # kernels (agg mode 1: a different implementation of the same recurrence, itself checked against the oracle
    # in tests/) on a second plan holding the same volumes
    got = [plan.download(f) for f in check_frames]
    with EpiPlan(W, H, D, len(check_frames), paths=PATHS, device=local_rank) as ref:
        ref.set_penalties(P1, P2, VMAX)
        ref.set_agg_mode(1)
        for i, v in enumerate(check_vols):
            ref.upload_cost(i, v)
            ref.upload_offset(i, off)
        ref.run(stages)
        checked = all(np.array_equal(got[i][0], r[0]) and np.array_equal(got[i][1], r[1])
                      for i, r in enumerate(ref.download(i) for i in range(len(check_frames))))
        ref_kernel = ref.kernel_name
    del check_vols
    assert checked, "the timed pipeline's bestD/minC differ from the line kernels' on the same volumes"

    # stage timing with HIP events on the plan's own stream (the forked streams join it before the
    # second event), rank 0 reports
    agg_ms = plan.time(STAGE_AGGREGATE, warmup=1, iters=max(3, args.steps // 2))
    wta_ms = plan.time(STAGE_WTA, warmup=1, iters=max(3, args.steps // 2))

    try:
        free_b, total_b = torch.cuda.mem_get_info(local_rank)         # device-wide: the timed plan, its pipeline's volumes and the 16-frame check plan's leftovers
        hbm_used_gb = (total_b - free_b) / 1e9
    except Exception:
        hbm_used_gb = None
    if rank == 0:
        alg_bytes_launch = B * W * H * D * PATHS            # 1 byte of C per voxel-path
        # which kernels the stage is made of depends on the pipeline the plan picked for this batch size;
        # where the argmin is a kernel of its own (parallel sweeps, line kernels) it belongs to the timed stage
        stage_kernels = {
            "sweep16/nowrap": ("sweep_kernel<8,0> + sweep_kernel<8,2> + pair_ckpt_kernel<8,0> + pair_sum_kernel<8,0,false>", False),
            "sweep16par/nowrap": ("sweep_kernel<8,0> + sweep_kernel<8,1> + " + ("agg_packed_kernel<128,false,true> (the two along-x slots)" if B <= 5 else "pairx_ckpt_kernel<128> + pairx_sum_kernel<128>" if B <= 10 else "pair_ckpt_kernel<8,0> + pair_sum_kernel<8,0,false>") + " + wta_sweep_kernel<8>", True),
            "sweep16mid/nowrap": ("sweep_kernel<8,0> + sweep_kernel<8,1> (first halves) + sweep_kernel<8,3> + sweep_kernel<8,2> (final halves, WTA inside) + " + ("pairx_ckpt_kernel<128> + pairx_sum_kernel<128>" if B <= 10 else "pair_ckpt_kernel<8,0> + pair_sum_kernel<8,0,false>"), False),
            "pairs16/nowrap": ("pair_ckpt_kernel<8,0> + pair_sum_kernel<8,0,false> + pair_ckpt_kernel<8,1> + pair_sum_kernel<8,1,true>", False),
            "band16/nowrap": (f"band_kernel<8,0,8,{PATHS}> + band_kernel<8,2,8,{PATHS}>", False),
            "band16chain/nowrap": (f"band_kernel<8,0,8,{PATHS}> + band_kernel<8,2,8,{PATHS}> (one workgroup per band and frame)", False),
        }.get(plan.kernel_name, ("agg_packed_kernel<128,false,true> + wta_packed_kernel<8>", True))
        stage_time_ms = agg_ms + (wta_ms if stage_kernels[1] else 0.0)
        achieved = alg_bytes_launch / (stage_time_ms * 1e-3) / 1e9
        bpv, traffic_src = measured_traffic(plan.kernel_name, PATHS)
        out = result_line()
        out["config"]["hbm_in_use_GB_after_timed_loop"] = hbm_used_gb
        out.update({
            # band sweeps: the stage is two kernels back to back on the plan's stream (first pass, second pass + WTA),
            # each 4 voxel-paths per voxel: HIP events around the pair = the sum of their durations (rocprofv3 kernel
            # stats of this command: profiles/).  Block sweeps / pair pipeline (smaller batches): kernel types that run
            # concurrently on three streams, roofline over the stage, HIP events fork->join
            "roofline": {"bound": "hbm", "kernel": "aggregation stage: " + stage_kernels[0],
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": bpv * B * W * H * D if bpv else None, "traffic_source": traffic_src,
                         # the PMC figure is read from a committed profile, not measured in this run: it is this build's only if
                         # the library hash recorded with it equals this run's
                         "lib_sha16": lib_sha16(),
                         "traffic_stale": (traffic_src is not None and traffic_src.get("lib_sha16") != lib_sha16()) if bpv else None,
                         # the rate at which that traffic moved; the same access patterns without arithmetic reach 5.1-5.6 TB/s
                         # (tools/ubench/pattern_rates.hip, profiles/r02_ubench_pattern_rates.txt)
                         "traffic_GBps": (bpv * B * W * H * D / (stage_time_ms * 1e-3) / 1e9) if bpv else None,
                         "algorithmic_bytes": alg_bytes_launch, "stage_ms": agg_ms, "finish_ms": wta_ms},
            "checked": bool(checked),
            "check": f"frames {check_frames} of the timed plan == line kernels ({ref_kernel}) on the same volumes, bestD and minC, all pixels",
        })
        try:
            import ctypes as C
            g = C.c_double()
            # the achievable rate on this device: the library's own 16 B-per-lane copy kernel (read + written bytes)
            fsgm_amd._lib.check(plan.lib.fsgm_measure_copy_bandwidth2(local_rank, 1 << 30, 10, 0, C.byref(g)))
            out["roofline"]["copy_GBps_measured"] = g.value
            out["roofline"]["copy_kernel"] = "copy16_kernel (one 16-B element per thread, non-temporal), 1 GiB"
            out["roofline"]["frac_of_copy"] = achieved / g.value
            fsgm_amd._lib.check(plan.lib.fsgm_measure_copy_bandwidth2(local_rank, 1 << 30, 10, 1, C.byref(g)))
            out["roofline"]["memcpy_d2d_GBps_measured"] = g.value
        except Exception as e:                                # pragma: no cover
            out["roofline"]["copy_GBps_measured"] = None
        if world == 1 and not args.no_extras:
            # whole-MEX rate (reported separately, not the judged value): census x2 + cost fill
            # + 5x5 box + 8-path aggregation + WTA/sub-pixel/vz for the same resident frames, on the
            # survey's timing maps (Pd0 = (x+1, y+1), direction (-1, 0), offset 200) and on a direction field
            # with a random component per pixel (every lane of the census gather in its own cache line: the
            # worst case for the cost fill); this overwrites the synthetic volumes, so it runs last
            I1, I2 = synth.image_pair(W, H, D, seed=3)
            for key, kind in (("whole_mex", "axis"), ("whole_mex_radial_directions", "radial"), ("whole_mex_random_directions", "general")):
                pd0, nd, offg = synth.epi_maps(W, H, kind)
                for f in range(B):
                    plan.upload(f, I1, I2, pd0, nd, offg)
                all_ms = plan.time(STAGE_COST | STAGE_AGGREGATE | STAGE_WTA, warmup=1, iters=3)
                cost_ms = plan.time(STAGE_COST, warmup=1, iters=3)
                out[key] = {"ms_per_frame": all_ms / B, "frames_per_s": B / (all_ms * 1e-3), "cost_stage_ms_per_frame": cost_ms / B,
                            "stages": f"census x2, cost fill, box, aggregate({PATHS} paths), WTA", "inputs": "resident in HBM",
                            "maps": {"axis": "SURVEY 8(d) timing maps (horizontal epipolar lines)", "radial": "directions away from an epipole inside the image "
                                     "(a forward-moving camera: the field epipolar_geometry.m produces)", "general": "random direction per pixel"}[kind]}
        if world == 1 and not args.no_extras:
            # the boundary as a MATLAB caller feels it: host pointers in, host pointers out (pageable memory, PCIe
            # included; never `value`), one frame per call like epipolar_sgm_of.m:45, and 8 frames per call
            from fsgm_amd import calc_cost_sgm, calc_cost_sgm_batch
            plan.close()
            I1, I2 = synth.image_pair(W, H, D, seed=3)
            frames8 = [(I1, I2) + synth.epi_maps(W, H, "general", seed=40 + s) for s in range(8)]
            f0 = frames8[0]
            calc_cost_sgm(f0[0], f0[1], D, VMAX, f0[2], f0[3], f0[4], P1, P2, paths=PATHS)
            t0 = time.perf_counter()
            for _ in range(10):
                calc_cost_sgm(f0[0], f0[1], D, VMAX, f0[2], f0[3], f0[4], P1, P2, paths=PATHS)
            one = (time.perf_counter() - t0) / 10 * 1e3
            calc_cost_sgm_batch(frames8, D, VMAX, P1, P2, paths=PATHS)
            t0 = time.perf_counter()
            for _ in range(3):
                calc_cost_sgm_batch(frames8, D, VMAX, P1, P2, paths=PATHS)
            eight = (time.perf_counter() - t0) / 3 * 1e3
            bytes_frame = 2 * W * H + 5 * 8 * W * H + 2 * 4 * W * H
            # the driver one level up (epipolar_sgm_of.m:33-51) with the three fp64 maps made on the device from F, H, the
            # epipole: 2 images up, flow (3 fp64 planes) and minC down
            from fsgm_amd import epipolar_sgm_of
            Fm, Hm, epi, direction = synth.epi_geometry(W, H, "forward")
            epipolar_sgm_of(I1, I2, Fm, Hm, epi, direction, D, VMAX, paths=PATHS)
            t0 = time.perf_counter()
            for _ in range(10):
                epipolar_sgm_of(I1, I2, Fm, Hm, epi, direction, D, VMAX, paths=PATHS)
            driver = (time.perf_counter() - t0) / 10 * 1e3
            # BASELINE configs[1]: one 320x240 call with D = 64 and the shipped 4 paths (the MEX plumbing case)
            s1, s2 = synth.image_pair(320, 240, 64, seed=4)
            smaps = synth.epi_maps(320, 240, "general", seed=41)
            calc_cost_sgm(s1, s2, 64, VMAX, *smaps, P1, P2, paths=4)
            t0 = time.perf_counter()
            for _ in range(20):
                calc_cost_sgm(s1, s2, 64, VMAX, *smaps, P1, P2, paths=4)
            small = (time.perf_counter() - t0) / 20 * 1e3
            out["host_call_ms"] = {"one_frame": one, "eight_frames": eight, "ms_per_frame_in_batch": eight / 8, "config2_320x240x64_4paths_one_frame": small,
                                   "pcie_bytes_per_frame": bytes_frame,
                                   "epipolar_driver_one_frame": driver, "epipolar_driver_pcie_bytes": 2 * W * H + 3 * 8 * W * H + 4 * W * H,
                                   "note": "fsgm_calc_cost_sgm(_batch)_host from pageable numpy buffers, whole call incl. H2D of 2 images + 5 fp64 map planes and D2H of bestD/minC; "
                                           "epipolar_driver: fsgm_epipolar_sgm_of_host, maps made on the device (2 images up, flow + minC down)"}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(PATHS=PATHS)
            out["cpu_baseline_all_cores"] = cpu_baseline_all_cores(PATHS=PATHS)
        print(json.dumps(out), flush=True)
    plan.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
