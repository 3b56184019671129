"""GPU tests of the packed line kernels and the packed WTA at the disparity ranges beyond 16 << k (agg_line_split: 48, 96, 192 as
12 costs a lane, 80 and 160 as 20, 112 and 224 as 28).  Every compared output is an integer array compared for equality with the
CPU oracle (pinned to the reference's compiled code at two of these ranges in tests/test_line_splits_cpu.py) or, where the oracle
has no such row, with the numpy restatements the adaptive-P2 and stereo tests use.  Every case names the pipeline it expects.

The two shapes, 37x21 and 13x26: a wave holds 16, 8 or 4 lines (64 / LPP) against 21, 37, 13 or 26 lines -- several waves and a
last partial group --, lengths that are no multiple of the prefetch depth 4, diagonals that re-enter at both borders with W > H and
W < H, and the mirrored pass.  The torch op: tests/test_gpu_line_splits_torch.py."""
import functools

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, synth
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_ALL, STAGE_WTA
from fsgm_amd.epi import auto_pipeline
from tests import adaptive_p2_restatement as A
from tests import mexharness as mh
from tests import stereo_restatement as R

pytestmark = pytest.mark.gpu

SPLITS = (48, 80, 96, 112, 160, 192, 224)
SHAPES = ((37, 21), (13, 26))
NOWRAP, WRAP = "packed16/nowrap", "packed16/wrap"
PENALTIES = {NOWRAP: (6, 64), WRAP: (100, 200)}


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


@functools.lru_cache(maxsize=None)
def _volume(W, H, D, kernel):
    """costs up to 24 for the no-wrap kernels, over the whole byte range for the wrapping ones (every mod-256 narrowing taken);
    planted pixels: best == D - 1 (the parabola reads the next pixel's d = 0), best == 1 and 0 (never refined), and the frame's
    last pixel with best == D - 1 (the word past the array: 0)"""
    hi = 24 if kernel == NOWRAP else 255
    Cv = synth.cost_volume(W, H, D, seed=W * 7 + D, cmax=24) if kernel == NOWRAP else synth.uniform_u8(W * 7 + D, (H, W, D))
    for (y, x), d in (((2, 3), D - 1), ((4, 5), 1), ((6, 7), 0), ((H - 1, W - 1), D - 1)):
        Cv[y, x, :] = hi
        Cv[y, x, d] = 0
    Cv.setflags(write=False)
    return Cv


@functools.lru_cache(maxsize=None)
def _offsets(W, H):
    off = synth.epi_maps(W, H, "general", seed=3)[2]
    off.setflags(write=False)
    return off


@functools.lru_cache(maxsize=None)
def _sums(W, H, D, kernel, paths):
    """the oracle's S for _volume, computed once and shared"""
    from oracle import pyoracle
    S = pyoracle.epi_aggregate(_volume(W, H, D, kernel), *PENALTIES[kernel], paths)
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("subpixel", (0, 1))
@pytest.mark.parametrize("kernel", (NOWRAP, WRAP))
@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("D", SPLITS)
def test_aggregation_and_wta_match_the_oracle(gpu_lib, oracle, D, W, H, paths, kernel, subpixel):
    """subpixel=1 with the vz -> disparity conversion, subpixel=0 without"""
    S, off = _sums(W, H, D, kernel, paths), _offsets(W, H)
    bd, mc = oracle.epi_wta(S, W, H, D, subpixel)
    if subpixel:
        bd = oracle.epi_vz_to_disp(bd, off, 0.3, D + 1)
    with EpiPlan(W, H, D, 1, paths=paths, subpixel=subpixel, vz_to_disp=subpixel) as plan:
        plan.set_penalties(*PENALTIES[kernel], 0.3)
        plan.upload_cost(0, _volume(W, H, D, kernel))
        plan.upload_offset(0, off)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == kernel
        gbd, gmc = plan.download(0)
    _eq(gmc, mc, "minC")
    _eq(gbd, bd, "bestD")


@pytest.mark.parametrize("kernel", (NOWRAP, WRAP))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("D", (48, 160, 224))                    # 3, 5 and 7 cost dwords a lane
def test_adaptive_p2_matches_the_restatement(gpu_lib, oracle, D, W, H, kernel):
    P1, P2 = PENALTIES[kernel]
    Cv = _volume(W, H, D, kernel)
    I1 = synth.uniform_u8(W + D, (H, W))                         # raw noise: most steps cross an intensity edge
    want = oracle.epi_wta(A.aggregate(Cv, I1, P1, P2, 8, 1), W, H, D, 1)
    with EpiPlan(W, H, D, 1, paths=8, vz_to_disp=0, adaptive_p2=1) as plan:
        plan.set_penalties(P1, P2, 0.3)
        plan.upload_cost(0, Cv)
        plan.upload_images(0, I1, I1)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == kernel
        got = plan.download(0)
        plan.set_adaptive_p2(0)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == kernel
        plain = plan.download(0)
    _eq(got[1], want[1], "minC")
    _eq(got[0], want[0], "bestD")
    _eq(plain[1], oracle.epi_wta(_sums(W, H, D, kernel, 8), W, H, D, 1)[1], "minC, adaptive off")
    assert (plain[1] != got[1]).any()                            # the switch does something on this frame


def test_batch_of_three_distinct_frames_through_one_plan(gpu_lib, oracle):
    """a wrong frame or direction stride of the path volumes shows"""
    W, H, D = 37, 21, 96
    frames = [synth.image_pair(W, H, D, seed=s) + synth.epi_maps(W, H, "general", seed=s) for s in (3, 4, 5)]
    with EpiPlan(W, H, D, 3, paths=8) as plan:
        plan.set_penalties(6, 64, 0.3)
        for f, fr in enumerate(frames):
            plan.upload(f, *fr)
        plan.run(STAGE_ALL)
        assert plan.kernel_name == NOWRAP
        got = [plan.download(f) for f in range(3)]
    for f, (I1, I2, pd0, nd, off) in enumerate(frames):
        bd, mc = oracle.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, 8)
        _eq(got[f][1], mc, f"minC of frame {f}")
        _eq(got[f][0], bd, f"bestD of frame {f}")


def test_calc_cost_sgm_with_the_forward_backward_check(gpu_lib, oracle):
    W, H, D = 37, 21, 80
    I1, I2 = synth.image_pair(W, H, D, seed=5)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=6)
    bd_idx, mc = oracle.epi_wta(oracle.epi_aggregate(oracle.epi_cost(I1, I2, D, 0.3, pd0, nd, off), 6, 64, 8), W, H, D, 1)
    conf, d2 = oracle.epi_fb_check(bd_idx, pd0, nd, off, 0.3, D + 1)
    assert auto_pipeline(W, H, D, 1, 8, 6, 64) == NOWRAP         # the one-shot call's plan is chosen by this function
    gbd, gmc, gconf, gd2 = fsgm_amd.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, paths=8, fb_check=1)
    _eq(gmc, mc, "minC")
    _eq(gbd, oracle.epi_vz_to_disp(bd_idx, off, 0.3, D + 1), "bestD")
    _eq(gd2, d2, "bestD2")
    _eq(gconf, conf, "conf")


@pytest.mark.parametrize("D,paths,direction,fb", [(192, 4, -1, 0), (96, 8, +1, 1)])
def test_stereo_sgm_matches_the_restatement(gpu_lib, oracle, D, paths, direction, fb):
    W, H = 40, 12
    L, Rt = synth.image_pair(W, H, 16, seed=D)
    if direction > 0:
        L, Rt = Rt, L
    Cv = R.box_mean(R.rectified_raw_cost(L, Rt, D, direction))
    wbd, wmc = oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, paths), W, H, D, 1)
    assert auto_pipeline(W, H, D, 1, paths, 6, 64) == NOWRAP
    got = fsgm_amd.stereo_sgm(L, Rt, D) if (paths, direction, fb) == (4, -1, 0) else \
        fsgm_amd.stereo_sgm(L, Rt, D, paths=paths, direction=direction, fb_check=fb)
    _eq(got[1], wmc, "minC")
    _eq(got[0], wbd, "disp")
    if fb:
        wconf, wd2 = R.linear_fb_check(wbd, *R.rectified_maps(W, H, direction))
        _eq(got[3], wd2, "disp2")
        _eq(got[2], wconf, "conf")


def test_mex_gateway(gpu_lib, oracle):
    W, H, D = 37, 21, 48
    I1, I2 = synth.image_pair(W, H, D, seed=2)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=4)
    bd, mc = oracle.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, 4)
    assert auto_pipeline(W, H, D, 1, 4, 6, 64) == NOWRAP
    outs, _ = mh.call("calc_cost_sgm", 2, I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    _eq(outs[1], mc, "minC")
    _eq(outs[0], bd, "bestD")


@pytest.mark.parametrize("paths", (4, 8))
def test_sum_tap(gpu_lib, oracle, paths):
    W, H, D = 13, 26, 112
    with EpiPlan(W, H, D, 1, paths=paths) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload_cost(0, _volume(W, H, D, NOWRAP))
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == NOWRAP
        _eq(plan.download_sum(0), _sums(W, H, D, NOWRAP, paths)[:-1].reshape(H, W, D), "S")


def test_forced_fused_modes_leave_the_line_kernels_in_place(gpu_lib, oracle):
    W, H, D = 37, 21, 192
    bd, mc = oracle.epi_wta(_sums(W, H, D, NOWRAP, 8), W, H, D, 1)
    with EpiPlan(W, H, D, 1, paths=8, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload_cost(0, _volume(W, H, D, NOWRAP))
        for mode in (2, 3, 4, 5, 6):
            plan.set_agg_mode(mode)
            assert plan.kernel_name == NOWRAP, mode
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            gbd, gmc = plan.download(0)
            _eq(gmc, mc, f"minC, mode {mode}")
            _eq(gbd, bd, f"bestD, mode {mode}")
