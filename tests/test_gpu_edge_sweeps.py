"""Seeded sweeps of the layers built on the four MEX cores -- the post-processing chain of test.m:45-50, vmf, the two pyramidal
drivers and the epipolar maps / epipolar_flow_pp -- against the CPU oracle, on edge-value inputs (tests/edge_inputs.py): shapes on
the tile and scan-chunk edges, ties on maxDiff, regions one pixel either side of maxSpeckleSize, +-0.0, +Inf, subnormals, NaN rows /
columns / frames, targets on the border and on round-half points, contention on one cell, epipoles on a pixel.  Everything is
compared exactly (NaN positions, then values).  FSGM_FUZZ_SEEDS=N runs every sweep with N seeds (a soak run)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, PostPlan, PyramidPlan, NgPyramidPlan  # noqa: E402  (torch first, then the library)
from fsgm_amd import synth  # noqa: E402
from tests import edge_inputs as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_SOAK = int(os.environ.get("FSGM_FUZZ_SEEDS", "0"))


def _seeds(default):
    return range(_SOAK if _SOAK > 0 else default)


def _same(a, b, msg=""):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    np.testing.assert_array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0), err_msg=msg)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


NAMES = ("filterD1", "filterD2", "filterdisparites")


# ============================================================================================== A. post-processing chain
@pytest.mark.parametrize("seed", _seeds(16))
def test_post_random_configs(gpu_lib, oracle, seed):
    r = E.rng(1000 + seed)
    W, H, N = E.post_shape(r)
    maxDiff, maxSize, vMax, n, dMax = E.post_params(r)
    D1 = E.post_maps(r, W, H, N, maxSize, vMax, n)
    Pd0, nd, O = E.post_geometry(r, W, H, N)
    cfg = f"seed {seed} W{W} H{H} N{N} maxDiff {maxDiff} maxSize {maxSize} vMax {vMax} n {n} dMax {dMax}"
    want = []
    with np.errstate(all="ignore"):
        for f in range(N):
            msg = f"{cfg} frame {f}"
            out, labels = fsgm_amd.speckle_filter(D1[f], maxDiff, maxSize)
            wout, wlabels = oracle.speckle_filter(D1[f], maxDiff, maxSize)
            _same(out, wout, msg + " speckle_filter")
            np.testing.assert_array_equal(labels, wlabels, err_msg=msg + " speckle_filter labels")
            wD2 = oracle.calc_disp_from_first(D1[f], Pd0[f], nd[f], O[f], vMax, n)
            _same(fsgm_amd.calc_disp_from_first(D1[f], Pd0[f], nd[f], O[f], vMax, n), wD2, msg + " calc_disp_from_first")
            _same(fsgm_amd.forward_backward_check(D1[f], wD2, Pd0[f], nd[f], O[f], vMax, n),
                  oracle.forward_backward_check(D1[f], wD2, Pd0[f], nd[f], O[f], vMax, n), msg + " forward_backward_check")
            _same(fsgm_amd.scanline_in_fill(D1[f]), oracle.scanline_in_fill(D1[f]), msg + " scanline_in_fill")
            _same(fsgm_amd.vzInd2Disp(D1[f], O[f], vMax, n), oracle.vzind2disp(D1[f], O[f], vMax, n), msg + " vzInd2Disp")
            want.append(oracle.postprocess(D1[f], Pd0[f], nd[f], O[f], vMax, n, dMax))
    # the chain through its four entry points
    f = int(r.randint(0, N))
    for g, w, name in zip(fsgm_amd.epi_postprocess(D1[f], Pd0[f], nd[f], O[f], vMax, n, dMax), want[f], NAMES):
        _same(g, w, f"{cfg} frame {f} single map {name}")
    with PostPlan(W, H) as plan:
        plan.upload(D1[f], Pd0[f], nd[f], O[f])
        for rep in range(2):
            plan.run(vMax, n, dMax)
            for g, w, name in zip(plan.download(), want[f], NAMES):
                _same(g, w, f"{cfg} frame {f} PostPlan run {rep} {name}")
    got = fsgm_amd.epi_postprocess_batch(D1, Pd0, nd, O, vMax, n, dMax)
    for f in range(N):
        for g, w, name in zip(got, want[f], NAMES):
            _same(g[f], w, f"{cfg} frame {f} host batch {name}")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        args = [_t(a) * 1.0 for a in (D1, Pd0, nd, O)]
        *dev, st = torch_ops.epi_postprocess(*args, vMax, n, dMax, return_status=True)
        dev = [d.clone() for d in dev]
    s.synchronize()
    assert int(st.item()) == 0, cfg
    for f in range(N):
        for g, w, name in zip(dev, want[f], NAMES):
            _same(_n(g)[f], w, f"{cfg} frame {f} torch op {name}")


def test_minus_zero_offers_keep_their_pixels(gpu_lib, oracle):
    """calc_disp_from_first.m:24-46: a cell whose only offers are -0.0 takes -0.0 (it starts at -1 and -1 < -0.0), so
    forward_backward_check keeps the pixels that look at it (:27).  The maximum on bit patterns must see -0.0 as +0.0."""
    W, H, vMax, n = 9, 4, 0.3, 65.0
    D1 = np.full((H, W), 2.0)
    D1[1:3, 2:6] = -0.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Pd0 = np.stack([xx + 1.0, yy + 1.0])
    nd, O = np.zeros((2, H, W)), np.full((H, W), 3.0)           # every pixel offers to its own cell only
    D2 = fsgm_amd.calc_disp_from_first(D1, Pd0, nd, O, vMax, n)
    wD2 = oracle.calc_disp_from_first(D1, Pd0, nd, O, vMax, n)
    assert (wD2[2, 3:6] == 0.0).all()                            # offers go to the cell and its right / lower neighbours
    _same(D2, wD2)
    chk = fsgm_amd.forward_backward_check(D1, D2, Pd0, nd, O, vMax, n)
    _same(chk, oracle.forward_backward_check(D1, wD2, Pd0, nd, O, vMax, n))
    assert not np.isnan(chk[1:3, 2:6]).any()
    big = np.tile(D1, (12, 12))                                  # the chain: a region of -0.0 large enough for both speckle passes
    W2, H2 = big.shape[1], big.shape[0]
    yy, xx = np.mgrid[0:H2, 0:W2].astype(np.float64)
    Pd0, O = np.stack([xx + 1.0, yy + 1.0]), np.full((H2, W2), 3.0)
    big[:] = 2.0
    big[10:30, 10:40] = -0.0
    nd = np.ones((2, H2, W2))
    nd[:, 10:30, 10:40] = 0.0
    want = oracle.postprocess(big, Pd0, nd, O, vMax, n, 64)
    assert not np.isnan(want[0][10:30, 10:40]).any()
    for g, w, name in zip(fsgm_amd.epi_postprocess(big, Pd0, nd, O, vMax, n, 64), want, NAMES):
        _same(g, w, name)


@pytest.mark.parametrize("seed", _seeds(8))
def test_vmf_random_configs(gpu_lib, oracle, seed):
    r = E.rng(1500 + seed)
    W, H = E.pick_size(r, 1, 150, (1, 2, 3, 4, 5, 63, 64, 65)), E.pick_size(r, 1, 100, (1, 2, 3, 4, 5, 6))
    N, ch = int(r.randint(1, 5)), int(r.randint(1, 4))
    flow = E.vmf_flows(r, W, H, N, ch)
    cfg = f"seed {seed} W{W} H{H} N{N} ch{ch}"
    want = [oracle.vmf(flow[f]) for f in range(N)]
    got = _n(torch_ops.vmf(_t(flow)))
    for f in range(N):
        _same(fsgm_amd.vmf(flow[f]), want[f], f"{cfg} frame {f} host")
        _same(got[f], want[f], f"{cfg} frame {f} torch op")


def test_vmf_nan_window(gpu_lib, oracle):
    """A NaN in the window is ordered above every number (never dropped, no neighbour counted twice); the median is NaN only when
    fewer than 13 of the 25 values are numbers."""
    flow = np.arange(1.0, 50.0).reshape(1, 7, 7)
    flow[0, 3, :] = np.nan
    got = fsgm_amd.vmf(flow)
    assert got[0, 3, 3] == 32.0
    _same(got, oracle.vmf(flow))
    flow[0, 1:3, 1:6] = np.nan
    got = fsgm_amd.vmf(flow)
    assert np.isnan(got[0, 3, 3])
    _same(got, oracle.vmf(flow))


def _tiny_templates():
    """Six 25x4 maps (100 pixels: the first speckle pass keeps a 100-pixel region) with identity-like geometry."""
    r = E.rng(77)
    W, H, T = 25, 4, 6
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    D1 = np.empty((T, H, W))
    Pd0 = np.broadcast_to(np.stack([xx + 1.0, yy + 1.0]), (T, 2, H, W)).copy()
    nd = np.ones((T, 2, H, W))
    O = np.zeros((T, H, W))
    for t in range(T):
        D1[t] = 10.0 + t + np.round(r.rand(H, W) * 4) / 4
        D1[t][r.rand(H, W) < 0.1 * max(t - 2, 0)] = np.nan
        O[t] = r.rand(H, W) * t / 2
        nd[t, 0] = np.cos(t * 0.7)
        nd[t, 1] = np.sin(t * 0.7)
    D1[5, 1] = np.nan
    D1[2] -= 12.0                                                # values 0..1, a column of -0.0: one region of 100 pixels
    D1[2, :, 3] = -0.0
    return D1, Pd0, nd, O


def test_more_than_65535_frames(gpu_lib, oracle):
    """70 000 frames: every frame-indexed launch is split at 65535 frames (blockIdx.z).  Frames are copies of six templates, so the
    oracle runs once per template."""
    D1t, Pd0t, ndt, Ot = _tiny_templates()
    T, N, vMax, n, dMax = D1t.shape[0], 70_000, 0.3, 65.0, 64
    idx = np.arange(N) % T
    idx[65535:65541] = np.arange(T)[::-1]                        # the frames right after the split differ from their neighbours
    want = [oracle.postprocess(D1t[t], Pd0t[t], ndt[t], Ot[t], vMax, n, dMax) for t in range(T)]
    assert any(not np.isnan(w[0]).all() for w in want)
    maps = [a[idx] for a in (D1t, Pd0t, ndt, Ot)]

    def check(got, what):
        for t in range(T):
            sel = idx == t
            for g, w, name in zip(got, want[t], NAMES):
                _same(g[sel], np.broadcast_to(w, (int(sel.sum()),) + w.shape), f"{what} template {t} {name}")

    check(fsgm_amd.epi_postprocess_batch(*maps, vMax, n, dMax), "host batch")
    check([_n(g) for g in torch_ops.epi_postprocess(*[_t(a) for a in maps], vMax, n, dMax, check=True)], "torch op")
    del maps
    flows = np.stack([D1t[:, :1, :2], np.flip(D1t[:, 2:3, 5:7], -1)], axis=1)        # (T, 2, 1, 2): 140 000 planes
    flows[3, 0, 0, 0] = np.nan
    wv = [oracle.vmf(flows[t]) for t in range(T)]
    got = _n(torch_ops.vmf(_t(flows[idx])))
    for t in range(T):
        sel = idx == t
        _same(got[sel], np.broadcast_to(wv[t], (int(sel.sum()),) + wv[t].shape), f"vmf template {t}")


# ============================================================================================== B. pyramidal drivers
def _pyr_shape(r):
    W = E.pick_size(r, 1, 140, (1, 2, 3, 5, 7, 9, 31, 33, 63, 65))
    H = E.pick_size(r, 1, max(1, min(140, 6000 // W)), (1, 2, 3, 5, 7, 9, 31, 33))
    return W, H


def _depth(W, H):
    d = 1
    while max(W, H) > 1:
        W, H, d = (W + 1) // 2, (H + 1) // 2, d + 1
    return d


def _pyr_levels(r, W, H):
    d = _depth(W, H)
    return int(r.randint(1, d + 1)) if r.rand() < 0.8 else int(min(16, d + r.randint(1, 4)))


def _pyr_penalties(r):
    if r.rand() < 0.5:
        return int(r.randint(0, 20)), int(r.randint(0, 90))
    return int(r.randint(0, 256)), int(r.randint(0, 256))          # beyond the no-wrap budget, P1 > P2 now and then


@pytest.mark.parametrize("seed", _seeds(10))
def test_pyramidal_sgm_random_configs(gpu_lib, oracle, seed):
    r = E.rng(2000 + seed)
    W, H = _pyr_shape(r)
    numPyd, ch = _pyr_levels(r, W, H), int(r.choice([1, 3]))
    P1, P2 = _pyr_penalties(r)
    o = dict(P1=P1, P2=P2, aggHalfWinSize=int(r.randint(0, 4)), verSearchHalfWinSize=int(r.randint(0, 7)),
             horSearchHalfWinSize=int(r.randint(0, 7)), enableDiagonal=int(r.rand() < 0.7), totalPass=int(r.randint(1, 4)),
             adaptiveP2=int(r.rand() < 0.4))
    I0, I1 = E.image_pair(r, W, H, ch, seed=seed)
    cfg = f"seed {seed} W{W} H{H} ch{ch} numPyd {numPyd} {o}"
    want_mv, want_minC, want_lv = oracle.pyramidal_sgm(I0, I1, numPyd, o["P1"], o["P2"], o["aggHalfWinSize"], o["verSearchHalfWinSize"],
                                                       o["horSearchHalfWinSize"], o["enableDiagonal"], o["totalPass"], o["adaptiveP2"])
    mv, mvPyd, minC = fsgm_amd.pyramidal_sgm(I0, I1, numPyd, **o)
    for l in range(numPyd - 1, -1, -1):
        np.testing.assert_array_equal(mvPyd[l], want_lv[l], err_msg=f"{cfg} level {l + 1}")
    np.testing.assert_array_equal(mv, want_mv, err_msg=cfg)
    np.testing.assert_array_equal(minC, want_minC, err_msg=cfg)
    if seed % 4 == 1:                                            # a batch through one plan = single calls
        B = int(r.randint(2, 5))
        pairs = [(I0, I1)] + [E.image_pair(r, W, H, ch, seed=seed * 10 + f) for f in range(1, B)]
        with PyramidPlan(W, H, ch, numPyd, batch=B, **o) as plan:
            for f, (a, b) in enumerate(pairs):
                plan.upload(a, b, frame=f)
            plan.run()
            for f, (a, b) in enumerate(pairs):
                one = (mv, mvPyd, minC) if f == 0 else fsgm_amd.pyramidal_sgm(a, b, numPyd, **o)
                for l in range(numPyd, 0, -1):
                    g, gm = plan.download(l, frame=f)
                    np.testing.assert_array_equal(g, one[1][l - 1], err_msg=f"{cfg} batch {B} frame {f} level {l}")
                np.testing.assert_array_equal(gm, one[2], err_msg=f"{cfg} batch {B} frame {f} minC")
    if seed % 4 == 2:                                            # the torch op = the host call
        dmv, dminC = torch_ops.pyramidal_sgm(_t(I0), _t(I1), numPyd, check=True, **o)
        np.testing.assert_array_equal(_n(dmv), mv, err_msg=cfg + " torch op")
        np.testing.assert_array_equal(_n(dminC), minC, err_msg=cfg + " torch op")


@pytest.mark.parametrize("seed", _seeds(10))
def test_pyramidal_sgm_ng_random_configs(gpu_lib, oracle, seed):
    r = E.rng(2500 + seed)
    W, H = _pyr_shape(r)
    numPyd, ch = _pyr_levels(r, W, H), int(r.choice([1, 3]))
    P1, P2 = _pyr_penalties(r)
    o = dict(P1=P1, P2=P2, halfSearchWinSize=int(r.choice([0, 1, 1, 2])), aggSize=int(r.randint(0, 6)), subPixelRefine=int(r.rand() < 0.5))
    I0, I1 = E.image_pair(r, W, H, ch, seed=seed + 300)
    cfg = f"seed {seed} W{W} H{H} ch{ch} numPyd {numPyd} {o}"
    want, want_minC = E.oracle_pyramidal_ng(oracle, I0, I1, numPyd, o["halfSearchWinSize"], o["aggSize"], o["subPixelRefine"], P1, P2)
    flow, flows, minC = fsgm_amd.pyramidal_sgm_ng(I0, I1, numPyd, **o)
    assert len(flows) == numPyd
    for k, (g, w) in enumerate(zip(flows, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{cfg} level {numPyd - k}")
    np.testing.assert_array_equal(minC, want_minC, err_msg=cfg)
    np.testing.assert_array_equal(flow, want[-1], err_msg=cfg)
    if seed % 4 == 1:
        B = int(r.randint(2, 5))
        pairs = [(I0, I1)] + [E.image_pair(r, W, H, ch, seed=seed * 10 + f) for f in range(1, B)]
        with NgPyramidPlan(W, H, ch, numPyd, batch=B, **o) as plan:
            for f, (a, b) in enumerate(pairs):
                plan.upload(a, b, frame=f)
            plan.run()
            for f, (a, b) in enumerate(pairs):
                one = (flow, flows, minC) if f == 0 else fsgm_amd.pyramidal_sgm_ng(a, b, numPyd, **o)
                for l in range(numPyd, 0, -1):
                    g, gm = plan.download(l, frame=f)
                    np.testing.assert_array_equal(g, one[1][numPyd - l], err_msg=f"{cfg} batch {B} frame {f} level {l}")
                np.testing.assert_array_equal(gm, one[2], err_msg=f"{cfg} batch {B} frame {f} minC")
    if seed % 4 == 2:
        dfl, dminC = torch_ops.pyramidal_sgm_ng(_t(I0), _t(I1), numPyd, check=True, **o)
        np.testing.assert_array_equal(_n(dfl), flow, err_msg=cfg + " torch op")
        np.testing.assert_array_equal(_n(dminC), minC, err_msg=cfg + " torch op")


# 3+ frames of 9 candidates: the grid kernel, which would ask for 280 672 bytes of LDS there (28 lines a workgroup), is no member of
# the matcher set below 16 candidates (ng_matcher_set); tests/test_gpu_ng_forms.py runs every form at this window
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_ng_batch_half0(gpu_lib, oracle, B):
    """halfSearchWinSize 0 on a batch of B frames, through NgPyramidPlan and the batched single-level call, against the oracle."""
    r = E.rng(4000 + B)
    W, H, numPyd = 13, 9, 2
    o = dict(P1=6, P2=32, halfSearchWinSize=0, aggSize=2, subPixelRefine=1)
    pairs = [E.image_pair(r, W, H, 1, seed=40 + f) for f in range(B)]
    want = [E.oracle_pyramidal_ng(oracle, a, b, numPyd, 0, 2, 1, 6, 32) for a, b in pairs]
    mvs = [np.ascontiguousarray(synth.hint_map(W, H, "int", seed=f, amp=2.0)) for f in range(B)]
    want1 = [oracle.calc_pyd_cost_sgm_ng(a, b, mv, 0, 2, 1, 6, 32) for (a, b), mv in zip(pairs, mvs)]
    got1 = fsgm_amd.calc_pyd_cost_sgm_ng_batch([(a, b, mv) for (a, b), mv in zip(pairs, mvs)], 0, 2, 1, 6, 32)
    for f in range(B):
        np.testing.assert_array_equal(got1[f][0], want1[f][0], err_msg=f"batch {B} frame {f} single level minC")
        np.testing.assert_array_equal(got1[f][1], want1[f][1], err_msg=f"batch {B} frame {f} single level flow")
    with NgPyramidPlan(W, H, 1, numPyd, batch=B, **o) as plan:
        for f, (a, b) in enumerate(pairs):
            plan.upload(a, b, frame=f)
        plan.run()
        for f in range(B):
            for l in range(numPyd, 0, -1):
                g, gm = plan.download(l, frame=f)
                np.testing.assert_array_equal(g, want[f][0][numPyd - l], err_msg=f"batch {B} frame {f} level {l}")
            np.testing.assert_array_equal(gm, want[f][1], err_msg=f"batch {B} frame {f} minC")


# ============================================================================================== C. epipolar maps, flow_pp
@pytest.mark.parametrize("seed", _seeds(10))
def test_epipolar_random_geometries(gpu_lib, oracle, seed):
    r, W, H, D, vMax, paths, ch, B, geos, pairs = E.epi_random_case(seed, oracle)
    cfg = f"seed {seed} W{W} H{H} D{D} vMax {vMax} paths {paths} ch{ch} B{B} epipoles {[g[4] for g in geos]}"
    for f, g in enumerate(geos):
        msg = f"{cfg} frame {f} epipole {g[2]} direction {g[3]}"
        with np.errstate(all="ignore"):
            want = oracle.epipolar_maps(*g[:4], W, H)
        for a, w, name in zip(fsgm_amd.epipolar_maps(*g[:4], W, H), want, ("Pd0", "normlizeDirection", "Offset", "Rflow")):
            _same(a, w, f"{msg} epipolar_maps {name}")
    f = int(r.randint(0, B))
    wflow, wminC = oracle.epipolar_sgm_of(*pairs[f], *geos[f][:4], D, vMax, paths)
    gflow, gminC = fsgm_amd.epipolar_sgm_of(*pairs[f], *geos[f][:4], D, vMax, paths=paths)
    np.testing.assert_array_equal(gminC, wminC, err_msg=f"{cfg} frame {f} epipolar_sgm_of minC")
    _same(gflow, wflow, f"{cfg} frame {f} epipolar_sgm_of flow")
    want = [E.oracle_flow_pp_frame(oracle, a, b, g[:4], paths, D, vMax) for (a, b), g in zip(pairs, geos)]
    F, Hm, e, d = (list(x) for x in zip(*[g[:4] for g in geos]))
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    host = fsgm_amd.epipolar_flow_pp(I0, I1, F, Hm, e, d, D, vMax, paths=paths)
    dev = torch_ops.epipolar_flow_pp(_t(I0), _t(I1), F, Hm, e, d, D, vMax, paths=paths, return_status=True)
    assert int(dev[-1].item()) == 0, cfg
    dev = [_n(t) for t in dev[:-1]]
    for f in range(B):
        for k, name in enumerate(("flow", "flow2", "D1", "minC")):
            _same(host[k][f], want[f][k], f"{cfg} frame {f} host epipolar_flow_pp {name}")
            _same(dev[k][f], want[f][k], f"{cfg} frame {f} torch epipolar_flow_pp {name}")
