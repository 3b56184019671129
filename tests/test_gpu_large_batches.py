"""GPU cases of tests/large_batches.py: batched entries whose device arrays cross 2^32 (once 2^34) bytes, every frame's every
output against the same entry run in sub-batches that keep every array below 2^31 bytes -- the regime the rest of the suite pins
to the oracle -- and, once per family, the frame that straddles the mark and the last frame against the CPU oracle itself.

A wrapped load shows in a high frame, a wrapped store in a low one: all frames are compared.  Frames are distinct (host volumes:
a pool varied by a per-frame roll; device tensors: one seeded draw for the whole batch).  Each case reads the free memory first
and skips below its inventoried peak plus headroom; it drops its plans and tensors at the end."""
import functools
import gc
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import EpiPlan, synth, torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA  # noqa: E402
from fsgm_amd.epi import stereo_last_kernel  # noqa: E402
from fsgm_amd.sgm import last_kernel  # noqa: E402
from tests import large_batches as L  # noqa: E402
from tests import stereo_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c.id: c for c in L.cases()}
NOWRAP, WRAP = (6, 64), (100, 200)
CMAX = 24


def _ids(family):
    return [c.id for c in CASES.values() if c.family == family]


class _Resident:
    """Skip unless the case's peak plus headroom is free; on exit drop every cached plan and torch's cache, and print the wall
    time and the largest drop of free memory seen at the sample points."""

    def __init__(self, gpu_lib, case):
        self.lib, self.case = gpu_lib, case

    def __enter__(self):
        torch.cuda.synchronize()
        free, _ = torch.cuda.mem_get_info()
        need = L.peak(self.case) + L.HEADROOM
        if free < need:
            pytest.skip(f"{self.case.id}: needs {need / L.GIB:.1f} GiB free (peak {L.peak(self.case) / L.GIB:.1f} + headroom), "
                        f"{free / L.GIB:.1f} GiB are")
        self.free0, self.low, self.t0 = free, free, time.perf_counter()
        return self

    def sample(self):
        self.low = min(self.low, torch.cuda.mem_get_info()[0])

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.sample()
        self.lib.fsgm_shutdown()
        gc.collect()
        torch.cuda.empty_cache()
        print(f"\n[large-batch] {self.case.id}: n={self.case.n} {time.perf_counter() - self.t0:.1f} s, "
              f"free memory dropped by {(self.free0 - self.low) / L.GIB:.1f} GiB (inventory: {L.peak(self.case) / L.GIB:.1f})")
        return False


def _bad_frames(got, want):
    """indices of the frames in which two (n, ...) arrays differ"""
    return [f for f in range(len(want)) if not np.array_equal(got[f], want[f])]


def _same_bits(a, b):
    """frames in which two device tensors of one shape differ, bit for bit (uint32 / float64 compared as integers)"""
    v = torch.int64 if a.element_size() == 8 else torch.int32 if a.element_size() == 4 else torch.uint8
    diff = (a.view(v) != b.view(v)).flatten(1).any(1)
    return diff.nonzero().flatten().tolist()


# ---------------------------------------------------------------------------------------------- 1-3. resident plans on host volumes
@functools.lru_cache(maxsize=None)
def _pool(W, H, D):
    return tuple(synth.cost_volume(W, H, D, seed=31 + s, cmax=CMAX) for s in range(4))


def _volume(W, H, D, f):
    """frame f: volume f % 4 of the pool, rolled by a shift no other frame of that volume has"""
    j = f // 4 + 1
    return np.roll(_pool(W, H, D)[f % 4], (j // W, j % W), axis=(0, 1))


def _run_plan(W, H, D, paths, f0, n, P, mode):
    """(bestD, minC, kernel name) of frames f0 .. f0 + n - 1 through one resident plan: upload_cost -> run -> download"""
    with EpiPlan(W, H, D, n, paths=paths, vz_to_disp=0) as plan:
        plan.set_penalties(P[0], P[1], 0.3)
        plan.set_agg_mode(mode)
        for f in range(n):
            plan.upload_cost(f, _volume(W, H, D, f0 + f))
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        name = plan.kernel_name
        outs = [plan.download(f) for f in range(n)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), name


@functools.lru_cache(maxsize=None)
def _plan_reference(W, H, D, paths, n, P):
    """The same frames on the line kernels, in sub-batches whose dL stays below 2^31 bytes; shared by every mode of a shape"""
    lines = L.epi_plan_arrays(W, H, D, paths, "packed16/nowrap" if L.packed_lpp(D) else "generic")
    sb = L.sub_batch(lines)
    parts = [_run_plan(W, H, D, paths, f0, min(sb, n - f0), P, 1) for f0 in range(0, n, sb)]
    assert all(p[2] in L.LINE_PIPES for p in parts)
    bd, mc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    bd.setflags(write=False), mc.setflags(write=False)
    return bd, mc


PLAN_MODE = {"lines-p8-L": 1, "lines-p4-C": 1, "lines-p4-C-wrap": 1, "generic-d300": 0}
PLAN_ORACLE = ("fused-p8-m4", "lines-p8-L", "generic-d300")       # one case per family also against the CPU oracle


@pytest.mark.parametrize("cid", _ids("epi_plan/fused") + _ids("epi_plan/lines") + _ids("epi_plan/generic"))
def test_resident_plan(gpu_lib, oracle, cid):
    case = CASES[cid]
    W, H, D, paths, n = case.W, case.H, case.D, case.paths, case.n
    P = WRAP if cid.endswith("wrap") else NOWRAP
    mode = PLAN_MODE[cid] if cid in PLAN_MODE else int(cid.rsplit("-m", 1)[1])
    with _Resident(gpu_lib, case) as res:
        want = _plan_reference(W, H, D, paths, n, P)
        with EpiPlan(W, H, D, n, paths=paths, vz_to_disp=0) as plan:
            plan.set_penalties(P[0], P[1], 0.3)
            plan.set_agg_mode(mode)
            for f in range(n):
                plan.upload_cost(f, _volume(W, H, D, f))
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            assert plan.kernel_name == case.pipeline
            plan.sync()
            res.sample()
            bad = [f for f in range(n) if not all(np.array_equal(g, w[f]) for g, w in zip(plan.download(f), want))]
            straddling = {f: plan.download(f) for f in (case.mark // case.target_bpf, n - 1)} if cid in PLAN_ORACLE else {}
        assert not bad, f"{cid} ({case.pipeline}): {len(bad)} of {n} frames differ from the sub-batch runs, first {bad[:8]}"
        for f, (gbd, gmc) in straddling.items():                 # the large plan's own frames against the oracle
            S = oracle.epi_aggregate(_volume(W, H, D, f), P[0], P[1], paths)
            bd, mc = oracle.epi_wta(S, W, H, D, 1)
            assert np.array_equal(gbd, bd) and np.array_equal(gmc, mc), f"{cid}: frame {f} differs from the oracle"


# ---------------------------------------------------------------------------------------------- 4. the cost stage from images
@functools.lru_cache(maxsize=None)
def _images(W, H, n):
    pool = [synth.image_pair(W, H, 24, seed=70 + s) for s in range(8)]
    shift = lambda f: ((f // 8 + 1) // W, (f // 8 + 1) % W)      # noqa: E731  (no two frames of one pair share a shift)
    left = np.stack([np.roll(pool[f % 8][0], shift(f), axis=(0, 1)) for f in range(n)])
    right = np.stack([np.roll(pool[f % 8][1], shift(f), axis=(0, 1)) for f in range(n)])
    left.setflags(write=False), right.setflags(write=False)
    return left, right


STEREO_KW = {"cost-stereo-d256": dict(fb_check=1), "cost-stereo-d256-ru": dict(runner_up=True), "cost-stereo-d260": dict()}


@pytest.mark.parametrize("cid", list(STEREO_KW))
def test_stereo_sgm_from_images(gpu_lib, oracle, cid):
    case = CASES[cid]
    W, H, D, n, kw = case.W, case.H, case.D, case.n, STEREO_KW[cid]
    left, right = _images(W, H, n)
    with _Resident(gpu_lib, case) as res:
        parts = [fsgm_amd.stereo_sgm(left[a:a + case.sub_batch], right[a:a + case.sub_batch], D, *NOWRAP, paths=4, **kw)
                 for a in range(0, n, case.sub_batch)]
        want = [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]
        got = fsgm_amd.stereo_sgm(left, right, D, *NOWRAP, paths=4, **kw)
        assert stereo_last_kernel() == case.pipeline
        res.sample()
        for k, (g, w) in enumerate(zip(got, want)):
            bad = _bad_frames(g, w)
            assert not bad, f"{cid} output {k}: {len(bad)} of {n} frames differ from the sub-batch runs, first {bad[:8]}"
        if cid == "cost-stereo-d256":
            # the torch form on the same images, and two frames against the restatement of the cost stage + the oracle
            tl, tr = torch.from_numpy(left.copy()).to(DEV), torch.from_numpy(right.copy()).to(DEV)
            tgot = torch_ops.stereo_sgm(tl, tr, D, *NOWRAP, paths=4, check=True, **kw)
            assert stereo_last_kernel() == case.pipeline
            res.sample()
            for k, (g, w) in enumerate(zip(tgot, want)):
                bad = _bad_frames(g.cpu().numpy(), w)
                assert not bad, f"{cid} torch output {k}: {len(bad)} of {n} frames differ, first {bad[:8]}"
            del tgot, tl, tr
            for f in (case.mark // case.target_bpf, n - 1):
                Cv = R.box_mean(R.rectified_raw_cost(left[f], right[f], D, -1))
                bd, mc = oracle.epi_wta(oracle.epi_aggregate(Cv, *NOWRAP, 4), W, H, D, 1)
                assert np.array_equal(got[0][f], bd) and np.array_equal(got[1][f], mc), f"{cid}: frame {f} differs from the oracle"


def test_calc_cost_sgm_batch_from_images(gpu_lib):
    case = CASES["cost-vz-d128"]
    W, H, D, n = case.W, case.H, case.D, case.n
    left, right = _images(W, H, n)
    maps = [synth.epi_maps(W, H, "general", seed=7 + s) for s in range(4)]
    frames = [(left[f], right[f]) + tuple(maps[f % 4]) for f in range(n)]
    with _Resident(gpu_lib, case) as res:
        want = []
        for a in range(0, n, case.sub_batch):
            want += fsgm_amd.calc_cost_sgm_batch(frames[a:a + case.sub_batch], D, 0.3, *NOWRAP, paths=4)
        got = fsgm_amd.calc_cost_sgm_batch(frames, D, 0.3, *NOWRAP, paths=4)
        res.sample()
        # (the batch entry reports no kernel name: the library's own selection for this shape, batch and device)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert fsgm_amd.epi.auto_pipeline(W, H, D, n, 4, *NOWRAP, CMAX, cus) == case.pipeline
        bad = [f for f in range(n) if not all(np.array_equal(g, w) for g, w in zip(got[f], want[f]))]
        assert not bad, f"{len(bad)} of {n} frames differ from the sub-batch runs, first {bad[:8]}"


# ---------------------------------------------------------------------------------------------- 5. torch_ops.sgm on the caller's tensor
SGM_KW = {"sgm-dhw": dict(agg_mode=2, cost_bound=CMAX), "sgm-hwd": dict(agg_mode=2, cost_bound=CMAX),
          "sgm-dhw-exact": dict(arith="exact", cost_bound=CMAX), "sgm-hwd-ru": dict(runner_up=True, cost_bound=CMAX),
          "sgm-dhw-adaptive": dict(adaptive_p2=1, cost_bound=CMAX), "sgm-hwd-wrap": dict()}


@pytest.mark.parametrize("cid", list(SGM_KW))
def test_torch_sgm_on_the_callers_tensor(gpu_lib, oracle, cid):
    case = CASES[cid]
    W, H, D, n = case.W, case.H, case.D, case.n
    layout = "dhw" if "-dhw" in cid else "hwd"
    P = WRAP if cid.endswith("wrap") else NOWRAP
    kw = dict(SGM_KW[cid], layout=layout, paths=4)
    side = torch.cuda.Stream() if cid == "sgm-dhw" else torch.cuda.current_stream()
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(2024)
        with torch.cuda.stream(side):                            # made, used and compared on one stream, no wait between
            Cv = torch.randint(0, CMAX + 1, (n, D, H, W) if layout == "dhw" else (n, H, W, D), dtype=torch.uint8, device=DEV, generator=gen)
            assert Cv.numel() > L.MARK32 and Cv.is_contiguous()
            guide = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=DEV, generator=gen) if kw.get("adaptive_p2") else None
            sub = lambda t, a: None if t is None else t[a:a + case.sub_batch]  # noqa: E731
            parts = [torch_ops.sgm(Cv[a:a + case.sub_batch], *P, guide=sub(guide, a), **kw) for a in range(0, n, case.sub_batch)]
            want = [torch.cat([p[k] for p in parts]) for k in range(len(parts[0]))]
            del parts
            got = torch_ops.sgm(Cv, *P, guide=guide, return_status=True, **kw)
            name = last_kernel()
            bad = [_same_bits(g, w) for g, w in zip(got[:-1], want)]
        side.synchronize()
        res.sample()
        assert name == case.pipeline
        assert int(got[-1].item()) == 0
        assert len(want) == (3 if kw.get("runner_up") else 2)
        for k, b in enumerate(bad):
            assert not b, f"{cid} output {k}: {len(b)} of {n} frames differ from the sub-batch calls, first {b[:8]}"
        if cid == "sgm-dhw":
            for f in (case.mark // case.target_bpf, n - 1):
                vol = np.ascontiguousarray(Cv[f].permute(1, 2, 0).cpu().numpy())
                bd, mc = oracle.epi_wta(oracle.epi_aggregate(vol, *P, 4), W, H, D, 1)
                assert np.array_equal(got[0][f].cpu().numpy(), bd) and np.array_equal(got[1][f].cpu().numpy(), mc), f"frame {f} vs the oracle"
        del Cv, guide, want, got


def test_hwd_ingest_above_2_34_bytes(gpu_lib):
    """The straight copy's second launch (launch_sgm_ingest walks an hwd batch 2^34 bytes at a time), through the plan-level
    ingest: the whole of torch_ops.sgm at that size is above the memory cap (tests/large_batches.py sgm_over_2_34_peak).
    The coverage is SAMPLED: the plan offers no device-side view of dC, so dC is read back through download_cost for the frames
    around every mark, the first, the last and every 16th only -- a wrapped store into another frame would go unseen."""
    case = CASES["ingest-hwd-2^34"]
    W, H, D, n = case.W, case.H, case.D, case.n
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(34)
        src = torch.randint(0, CMAX + 1, (n, H, W, D), dtype=torch.uint8, device=DEV, generator=gen)
        assert src.numel() > L.MARK34
        with EpiPlan(W, H, D, n, vz_to_disp=0) as plan:
            st = plan.ingest_cost(src, layout="hwd", cost_bound=CMAX, return_status=True)
            torch.cuda.synchronize()
            res.sample()
            assert int(st.item()) == 0
            near = {m // case.target_bpf + d for m in (L.MARK31, L.MARK32, L.MARK34) for d in (-1, 0, 1)}
            frames = sorted(near | {0, n - 1} | set(range(0, n, 16)))
            bad = [f for f in frames if not np.array_equal(plan.download_cost(f), src[f].cpu().numpy())]
        assert not bad, f"{len(bad)} of {len(frames)} frames read back differ from the source, first {bad[:8]}"
        del src


# ---------------------------------------------------------------------------------------------- 8. the level-hint kernels
@pytest.mark.parametrize("cid", _ids("level_hints"))
def test_flow_level_hints(gpu_lib, cid):
    case = CASES[cid]
    W, H, n = case.W, case.H, case.n
    size = 3 if cid.endswith("median3") else 0
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(8)
        flow = torch.randn((n, 2, H, W), dtype=torch.float64, device=DEV, generator=gen) * 4.0
        flow[torch.rand((n, 2, H, W), device=DEV, generator=gen) < 0.05] = float("nan")
        want = torch.cat([torch_ops.flow_level_hints(flow[a:a + case.sub_batch], size) for a in range(0, n, case.sub_batch)])
        got = torch_ops.flow_level_hints(flow, size)
        assert got.shape == (n, 2, 2 * H, 2 * W) and got.numel() * 8 > L.MARK32
        bad = _same_bits(got, want)
        res.sample()
        assert not bad, f"{cid}: {len(bad)} of {n} frames differ from the sub-batch calls, first {bad[:8]}"
        if size == 0:                                            # the plain form against its definition: 2 * nearest-neighbour upsampling
            f = case.mark // case.target_bpf
            for k in (f, n - 1):
                up = (2.0 * flow[k]).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
                assert not _same_bits(got[k][None], up[None]), f"frame {k}"
        del flow, want, got


# ---------------------------------------------------------------------------------------------- 6. torch_ops.sgm2d on the caller's tensor
@pytest.mark.parametrize("cid", _ids("sgm2d_device"))
def test_torch_sgm2d_on_the_callers_tensor(gpu_lib, cid):
    from fsgm_amd.sgm2d import last_kernel as last_kernel2d
    case = CASES[cid]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    layout = "hwd" if "-hwd" in cid else "dhw_yx"
    kw = dict(layout=layout, cost_bound=CMAX, return_flow=True, arith="exact" if cid.endswith("exact") else "wrap")
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(6)
        costs = torch.randint(0, CMAX + 1, (n, H, W, 81) if layout == "hwd" else (n, 81, H, W), dtype=torch.uint8, device=DEV, generator=gen)
        hints = torch.round(torch.randn((n, 2, H + 1, W + 2), dtype=torch.float64, device=DEV, generator=gen) * 12.0) / 4.0
        assert costs.numel() > L.MARK32
        got = torch_ops.sgm2d(costs, 4, 4, 6, 32, hints=hints, return_status=True, **kw)
        name = last_kernel2d()
        torch.cuda.synchronize()
        res.sample()
        assert int(got[-1].item()) == 0
        bad = [[] for _ in got[:-1]]
        for a in range(0, n, sb):                                # each sub-batch compared and dropped
            part = torch_ops.sgm2d(costs[a:a + sb], 4, 4, 6, 32, hints=hints[a:a + sb], **kw)
            assert last_kernel2d() == name
            for k, (g, w) in enumerate(zip(got[:-1], part)):
                bad[k] += [a + f for f in _same_bits(g[a:a + sb], w)]
        assert name == case.pipeline
        for k, b in enumerate(bad):
            assert not b, f"{cid} output {k} ({name}): {len(b)} of {n} frames differ from the sub-batch calls, first {b[:8]}"
        del costs, hints, got, part


# ---------------------------------------------------------------------------------------------- 7. post-processing on maps across 2^32 bytes
def _tile(pool, n):
    """(n, ..., H, W) on the device from a pool (P, ..., H, W): frame f is pool[f % P] rolled by a shift of its own"""
    P, H, W = pool.shape[0], pool.shape[-2], pool.shape[-1]
    f = torch.arange(n, device=pool.device)
    j = f // P + 1
    ys = (torch.arange(H, device=pool.device)[None, :] - (j // W % H)[:, None]) % H
    xs = (torch.arange(W, device=pool.device)[None, :] - (j % W)[:, None]) % W
    if pool.dim() == 3:
        return pool[(f % P)[:, None, None], ys[:, :, None], xs[:, None, :]]
    c = torch.arange(pool.shape[1], device=pool.device)
    return pool[(f % P)[:, None, None, None], c[None, :, None, None], ys[:, None, :, None], xs[:, None, None, :]]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_epi_postprocess_on_maps_across_4_gib(gpu_lib):
    from tests import edge_inputs as E
    case = CASES["post-chain"]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    r = E.rng(77)
    vMax, nn, dMax = 0.3, 65.0, 64.0
    with _Resident(gpu_lib, case) as res:
        D1 = _tile(_dev(E.post_maps(r, W, H, 8, 100.0, vMax, nn)), n)
        geo = E.post_geometry(r, W, H, 8)
        idx = torch.arange(n, device=DEV) % 8
        Pd0, nd, O = (_dev(g)[idx] for g in geo)
        assert D1.numel() * 8 > L.MARK32 and D1.numel() < L.MARK31
        got = torch_ops.epi_postprocess(D1, Pd0, nd, O, vMax, nn, dMax, return_status=True)
        torch.cuda.synchronize()
        res.sample()
        assert int(got[-1].item()) == 0
        bad = [[] for _ in got[:-1]]
        for a in range(0, n, sb):
            part = torch_ops.epi_postprocess(D1[a:a + sb], Pd0[a:a + sb], nd[a:a + sb], O[a:a + sb], vMax, nn, dMax)
            for k, (g, w) in enumerate(zip(got[:-1], part)):
                bad[k] += [a + f for f in _same_bits(g[a:a + sb], w)]
        for k, b in enumerate(bad):
            assert not b, f"output {k}: {len(b)} of {n} frames differ from the sub-batch calls, first {b[:8]}"
        del D1, Pd0, nd, O, got, part


def _flows(W, H, n):
    from tests import flow_pp_inputs as F
    pairs = [F.flow_pair(W, H, "general", seed=5 + 3 * s) for s in range(4)]
    return _tile(_dev(np.stack([p[0] for p in pairs])), n), _tile(_dev(np.stack([p[1] for p in pairs])), n)


def test_flow_fb_check_across_4_gib(gpu_lib):
    case = CASES["flow-fb-check"]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    with _Resident(gpu_lib, case) as res:
        f, b = _flows(W, H, n)
        assert f.numel() * 8 > L.MARK32 and f.numel() < L.MARK31
        got = torch_ops.flow_fb_check(f, b)
        res.sample()
        bad = []
        for a in range(0, n, sb):
            bad += [a + k for k in _same_bits(got[a:a + sb], torch_ops.flow_fb_check(f[a:a + sb], b[a:a + sb]))]
        assert not bad, f"{len(bad)} of {n} frames differ from the sub-batch calls, first {bad[:8]}"
        kept = ~torch.isnan(got[-1, 0])
        assert kept.any() and not kept.all()                     # the last frame has both kept and rejected pixels
        del f, b, got


@pytest.mark.parametrize("cid", ["flow-speckle", "flow-in-fill"])
def test_flow_host_forms_across_4_gib(gpu_lib, cid):
    fn = fsgm_amd.flow_speckle_filter if cid == "flow-speckle" else fsgm_amd.flow_in_fill
    case = CASES[cid]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    with _Resident(gpu_lib, case) as res:
        flow = _flows(W, H, n)[0].cpu().numpy()
        torch.cuda.empty_cache()
        assert flow.nbytes > L.MARK32
        got = fn(flow)
        res.sample()
        bad = []
        for a in range(0, n, sb):
            want = fn(flow[a:a + sb])
            bad += [a + k for k in range(len(want)) if not np.array_equal(got[a + k].view(np.int64), want[k].view(np.int64))]
        assert not bad, f"{cid}: {len(bad)} of {n} frames differ from the sub-batch calls, first {bad[:8]}"
        assert not np.array_equal(got[-1].view(np.int64), flow[-1].view(np.int64))   # the filter did something in the last frame


def test_uniqueness_filter_across_4_gib(gpu_lib):
    case = CASES["uniqueness"]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(9)
        m = torch.rand((n, H, W), dtype=torch.float64, device=DEV, generator=gen) * 64.0
        m[torch.rand((n, H, W), device=DEV, generator=gen) < 0.05] = float("nan")
        minC = torch.randint(0, 4000, (n, H, W), dtype=torch.int32, device=DEV, generator=gen)
        minC2 = (minC + torch.randint(0, 400, (n, H, W), dtype=torch.int32, device=DEV, generator=gen))
        minC2[torch.rand((n, H, W), device=DEV, generator=gen) < 0.02] = -1          # NO_RUNNER_UP
        minC, minC2 = minC.view(torch.uint32), minC2.view(torch.uint32)
        assert m.numel() * 8 > L.MARK32
        got = torch_ops.uniqueness_filter(m, minC, minC2, 10)
        res.sample()
        bad = []
        for a in range(0, n, sb):
            bad += [a + k for k in _same_bits(got[a:a + sb], torch_ops.uniqueness_filter(m[a:a + sb], minC[a:a + sb], minC2[a:a + sb], 10))]
        assert not bad, f"{len(bad)} of {n} frames differ from the sub-batch calls, first {bad[:8]}"
        # the rule itself on the straddling and the last frame: NaN where minC2 * 90 < minC * 100 and minC2 is a runner-up
        for f in (case.mark // case.target_bpf, n - 1):
            c, c2 = minC[f].view(torch.int32).to(torch.int64), minC2[f].view(torch.int32).to(torch.int64)
            rej = (c2 != -1) & (c2 * 90 < c * 100)
            want = torch.where(rej, torch.full_like(m[f], float("nan")), m[f])
            assert not _same_bits(got[f][None], want[None]), f"frame {f} against the rule"
        del m, minC, minC2, got


def test_stereo_fb_check_across_4_gib(gpu_lib):
    case = CASES["stereo-fb-check"]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    with _Resident(gpu_lib, case) as res:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(10)
        D1 = torch.round(torch.rand((n, H, W), dtype=torch.float64, device=DEV, generator=gen) * 16.0 * 4.0) / 4.0
        D1[torch.rand((n, H, W), device=DEV, generator=gen) < 0.05] = float("nan")
        assert D1.numel() * 8 > L.MARK32
        got = torch_ops.stereo_fb_check(D1, return_second=True, return_status=True)
        torch.cuda.synchronize()
        res.sample()
        assert int(got[-1].item()) == 0
        bad = [[], []]
        for a in range(0, n, sb):
            part = torch_ops.stereo_fb_check(D1[a:a + sb], return_second=True)
            for k in range(2):
                bad[k] += [a + f for f in _same_bits(got[k][a:a + sb], part[k])]
        for k, b in enumerate(bad):
            assert not b, f"output {k}: {len(b)} of {n} frames differ from the sub-batch calls, first {b[:8]}"
        del D1, got, part


# ---------------------------------------------------------------------------------------------- 8. the pyramid drivers
@pytest.mark.parametrize("cid", ["pyramid-pyd", "pyramid-ng"])
def test_pyramid_drivers(gpu_lib, cid):
    case = CASES[cid]
    W, H, n, sb = case.W, case.H, case.n, case.sub_batch
    fn = torch_ops.pyramidal_sgm if cid == "pyramid-pyd" else torch_ops.pyramidal_sgm_ng
    left, right = _images(W, H, n)
    with _Resident(gpu_lib, case) as res:
        I0, I1 = torch.from_numpy(left.copy()).to(DEV), torch.from_numpy(right.copy()).to(DEV)
        got = fn(I0, I1, 3, batch=True, return_status=True)
        torch.cuda.synchronize()
        res.sample()
        assert int(got[-1].item()) == 0
        for a in range(0, n, sb):
            part = fn(I0[a:a + sb], I1[a:a + sb], 3, batch=True, check=True)
            for k, (g, w) in enumerate(zip(got[:-1], part)):
                bad = _same_bits(g[a:a + sb], w)
                assert not bad, f"{cid} output {k}: frames {[a + f for f in bad[:8]]} differ from the sub-batch calls"
        del I0, I1, got, part


@pytest.mark.parametrize("size", [0, 3])
def test_flow_level_hints_more_frames_than_a_grid_dimension(gpu_lib, size):
    """65535 + 5 frames of 2 x 2 flow: the second launch of launch_pyr_upsample2 / launch_pyr_median_upsample2 (the frame is
    blockIdx.y / .z).  Against two calls that fit one launch each and, for the plain form, against its definition."""
    n, H, W = 65540, 2, 2
    gen = torch.Generator(device=DEV)
    gen.manual_seed(65)
    flow = torch.randn((n, 2, H, W), dtype=torch.float64, device=DEV, generator=gen) * 4.0
    flow[torch.rand((n, 2, H, W), device=DEV, generator=gen) < 0.05] = float("nan")
    got = torch_ops.flow_level_hints(flow, size)
    want = torch.cat([torch_ops.flow_level_hints(flow[:40000], size), torch_ops.flow_level_hints(flow[40000:], size)])
    bad = _same_bits(got, want)
    assert not bad, f"{len(bad)} of {n} frames differ from the two smaller calls, first {bad[:8]}"
    if size == 0:
        up = (2.0 * flow).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        assert not _same_bits(got, up)
