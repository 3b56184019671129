"""GPU tests of rectified stereo with a search range that starts at d_min (fsgm_epi_plan_set_d_min, fsgm_stereo_sgm_host_range,
fsgm_amd.stereo_sgm(..., d_min=)).  Every compared output is an integer array and is compared for equality: against the oracle on
the shifted maps (tests/stereo_range_restatement.py) and, where it covers the case, against the reference's own compiled linear
build (tests/golden/ref_mex_stereo_range.npz).  The torch op: tests/test_gpu_stereo_range_torch.py."""
import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, _lib, synth
from fsgm_amd._lib import FsgmError, STAGE_ALL, STAGE_COST
from tests import stereo_range_restatement as SR
from tests import stereo_restatement as R

pytestmark = pytest.mark.gpu
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
N_CASES = SR.golden_count()
OLD_MARKER = 512 << 8


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---------------------------------------------------------------------------------------------- the reference's own code
@pytest.mark.parametrize("i", range(N_CASES))
def test_stereo_range_matches_the_reference_on_the_shifted_maps(gpu_lib, i):
    c, (bestD, minC, conf, bestD2) = SR.golden_case(i)
    outs = fsgm_amd.stereo_sgm(c["I1"], c["I2"], c["D"], c["P1"], c["P2"], paths=c["paths"], direction=c["direction"], fb_check=c["fb"],
                               d_min=c["d_min"])
    assert outs[0].dtype == np.int32 and outs[1].dtype == np.uint32
    _eq(outs[1], minC, c["id"] + " minC")
    _eq(outs[0], SR.true_disp(bestD, c["d_min"]), c["id"] + " disp")
    if c["fb"]:
        assert outs[2].dtype == np.uint8 and outs[3].dtype == np.int32
        _eq(outs[2], conf, c["id"] + " conf")
        _eq(outs[3], SR.true_disp2(bestD2, c["d_min"]), c["id"] + " disp2")


# ---------------------------------------------------------------------------------------------- the cost stage, every form
# W = 61: one strip of 60 output columns plus one column, 130: three strips, the last partial, 59: less than a strip -- 61 and 130
# put the shift across strip aprons; d_min = -dMax - 3 and W + 5 make the whole window one clamped column (either image side,
# depending on the direction), -1 / 1 catch an off-by-one in the window's base.  dMax 16 .. 256: the fused cost kernel, and the
# raw-cost kernel + box under FSGM_COST_FUSED=0; 48, 100, 192: the raw-cost kernel + box always.
@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H", [7, 23])
@pytest.mark.parametrize("W", [61, 130, 59])
@pytest.mark.parametrize("D", [16, 32, 64, 128, 256, 48, 100, 192])
def test_shifted_cost_stage_and_outputs_match_the_oracle(gpu_lib, monkeypatch, D, W, H, direction):
    I1, I2 = synth.image_pair(W, H, min(D, 64), seed=D + W + H)
    fused_exists = D in (16, 32, 64, 128, 256)
    with EpiPlan(W, H, D, 1, sampling=_lib.SAMPLING_RECTIFIED, direction=direction) as plan:
        plan.set_penalties(6, 64)
        plan.upload_images(0, I1, I2)
        for d_min in (-D - 3, -17, -1, 1, 7, 63, W + 5):
            want = SR.oracle(I1, I2, D, direction, d_min)
            what = f"d_min {d_min}"
            plan.set_d_min(d_min)
            monkeypatch.setenv("FSGM_COST_FUSED", "1")
            plan.run(STAGE_ALL)
            Cv = plan.download_cost(0)
            _eq(Cv, want["C"], what + ": C")                     # every voxel
            bd, mc = plan.download(0)
            _eq(mc, want["minC"], what + ": minC")
            _eq(bd, want["bestD"], what + ": bestD (the plan's own outputs stay candidate indices * 256)")
            _eq(plan.download_sum(0), want["S"], what + ": S")
            if fused_exists:                                     # the two-kernel form must agree with the fused one bit for bit
                monkeypatch.setenv("FSGM_COST_FUSED", "0")
                plan.run(STAGE_COST)
                _eq(plan.download_cost(0), Cv, what + ": raw-cost + box kernels vs the fused kernel")


def test_set_d_min_is_for_rectified_plans_and_bounded(gpu_lib):
    with EpiPlan(24, 9, 16, 1, sampling=_lib.SAMPLING_RECTIFIED, direction=-1) as plan:
        for bad in (1025, -1025):
            with pytest.raises(FsgmError) as e:
                plan.set_d_min(bad)
            assert e.value.status == FSGM_ERR_INVALID
        plan.set_d_min(1024)
        plan.set_d_min(-1024)
    for sampling in (_lib.SAMPLING_VZ, _lib.SAMPLING_LINEAR):
        with EpiPlan(24, 9, 16, 1, sampling=sampling) as plan:
            with pytest.raises(FsgmError) as e:
                plan.set_d_min(3)
            assert e.value.status == FSGM_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- pairs that need the shift
@pytest.mark.parametrize("W,H,D,direction,d_min,s,seed", SR.SHIFT_CASES)
def test_a_disparity_outside_the_unshifted_range_is_found(gpu_lib, W, H, D, direction, d_min, s, seed):
    I1, I2 = SR.shifted_pair(W, H, s, direction, seed)
    disp, minC = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction, d_min=d_min)
    want = SR.oracle(I1, I2, D, direction, d_min)
    _eq(minC, want["minC"], "minC")
    _eq(disp, SR.true_disp(want["bestD"], d_min), "disp")
    m = abs(s) + 2
    inner = disp[:, m + 1:W - m - 1]
    assert (np.abs(inner - 256 * s) <= 256).mean() >= 0.5        # the true disparity, where the unshifted range cannot look
    d0, _ = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction)
    assert (d0.astype(np.int64)[:, m + 1:W - m - 1] != inner).mean() >= 0.5


# ---------------------------------------------------------------------------------------------- forward-backward check
@pytest.mark.parametrize("D,direction,d_min", [(64, -1, -17), (64, +1, 7), (64, -1, 1), (511, -1, -1), (511, +1, -300), (511, -1, 512)])
def test_range_fb_check_matches_the_oracle(gpu_lib, D, direction, d_min):
    W, H = 40, 26
    I1, I2 = synth.image_pair(W, H, 16, seed=D + d_min + 2000)
    disp, minC, conf, disp2 = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction, fb_check=1, d_min=d_min)
    want = SR.oracle(I1, I2, D, direction, d_min, fb_check=1)
    assert disp.dtype == np.int32 and disp2.dtype == np.int32 and conf.dtype == np.uint8
    _eq(minC, want["minC"], "minC")
    _eq(disp, SR.true_disp(want["bestD"], d_min), "disp")
    _eq(conf, want["conf"], "conf")
    _eq(disp2, SR.true_disp2(want["bestD2"], d_min), "disp2")
    _eq(disp2 == SR.INT32_MIN, want["bestD2"] == R.INVALID_DISPARITY, "the invalid marker")
    if d_min == 512:                                             # every sample clamps: index 0 wins, the true disparity is 512
        assert (disp == OLD_MARKER).any()                        # the old marker's value, here a valid disparity
        assert (disp2 == SR.INT32_MIN).all() and not conf.any()  # (every target lies outside the image)
    elif abs(d_min) < 20:
        assert (disp2 == SR.INT32_MIN).any() and (disp2 != SR.INT32_MIN).any() and conf.any()
    d1, m1 = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction, d_min=d_min)
    _eq(d1, disp, "disp with and without the check")
    _eq(m1, minC, "minC with and without the check")


def test_range_fb_check_rejects_dmax_512(gpu_lib):
    I1, I2 = synth.image_pair(9, 4, 16)
    with pytest.raises(FsgmError) as e:
        fsgm_amd.stereo_sgm(I1, I2, 512, fb_check=1, d_min=3)
    assert e.value.status == FSGM_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- batches, paths, modes
def test_range_batch_of_three_distinct_pairs(gpu_lib):
    W, H, D, d_min = 61, 9, 64, -17
    pairs = [synth.image_pair(W, H, 32, seed=70 + f) for f in range(3)]
    L, Rt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    disp, minC, conf, disp2 = fsgm_amd.stereo_sgm(L, Rt, D, fb_check=1, d_min=d_min)
    assert disp.shape == (3, H, W) and disp.dtype == np.int32
    for f, (I1, I2) in enumerate(pairs):
        want = SR.oracle(I1, I2, D, -1, d_min, fb_check=1)
        _eq(minC[f], want["minC"], f"minC of frame {f}")
        _eq(disp[f], SR.true_disp(want["bestD"], d_min), f"disp of frame {f}")
        _eq(conf[f], want["conf"], f"conf of frame {f}")
        _eq(disp2[f], SR.true_disp2(want["bestD2"], d_min), f"disp2 of frame {f}")
    assert (disp[0] != disp[1]).any() and (disp[1] != disp[2]).any()


@pytest.mark.parametrize("direction,d_min", [(-1, 7), (+1, -17)])
def test_range_with_eight_paths_adaptive_p2_and_forced_modes(gpu_lib, direction, d_min):
    W, H, D = 61, 23, 64
    I1, I2 = synth.image_pair(W, H, 32, seed=90 + d_min)
    want = SR.oracle(I1, I2, D, direction, d_min, paths=8)
    disp, minC = fsgm_amd.stereo_sgm(I1, I2, D, paths=8, direction=direction, d_min=d_min)
    _eq(minC, want["minC"], "8 paths: minC")
    _eq(disp, SR.true_disp(want["bestD"], d_min), "8 paths: disp")
    for paths in (4, 8):
        wa = SR.oracle(I1, I2, D, direction, d_min, paths=paths, adaptive=1)
        da, ma = fsgm_amd.stereo_sgm(I1, I2, D, paths=paths, direction=direction, adaptive_p2=1, d_min=d_min)
        _eq(ma, wa["minC"], f"adaptive P2, {paths} paths: minC")
        _eq(da, SR.true_disp(wa["bestD"], d_min), f"adaptive P2, {paths} paths: disp")
    got = {}
    for mode in (1, 2):                                          # per-direction line kernels, fused sweeps: identical results
        with EpiPlan(W, H, D, 1, paths=8, sampling=_lib.SAMPLING_RECTIFIED, direction=direction) as plan:
            plan.set_penalties(6, 64)
            plan.set_agg_mode(mode)
            plan.set_d_min(d_min)
            plan.upload_images(0, I1, I2)
            plan.run(STAGE_ALL)
            got[mode] = plan.download(0) + (plan.kernel_name,)
        _eq(got[mode][1], want["minC"], f"mode {mode}: minC")
        _eq(got[mode][0], want["bestD"], f"mode {mode}: bestD")
    assert got[1][2] != got[2][2], got                           # two pipelines ran


# ---------------------------------------------------------------------------------------------- the cached plan, d_min = 0
def test_cached_plan_keeps_no_shift_between_calls(gpu_lib):
    W, H, D = 61, 9, 32
    I1, I2 = synth.image_pair(W, H, D, seed=11)
    for fb in (0, 1):
        for d_min in (-17, 7, 7, 63):
            outs = fsgm_amd.stereo_sgm(I1, I2, D, fb_check=fb, d_min=d_min)
            want = SR.oracle(I1, I2, D, -1, d_min, fb_check=fb)
            _eq(outs[1], want["minC"], f"d_min {d_min}: minC")
            _eq(outs[0], SR.true_disp(want["bestD"], d_min), f"d_min {d_min}: disp")
            if fb:
                _eq(outs[3], SR.true_disp2(want["bestD2"], d_min), f"d_min {d_min}: disp2")
        # the same shape without d_min after them: what it always was
        outs = fsgm_amd.stereo_sgm(I1, I2, D, fb_check=fb)
        want = SR.oracle(I1, I2, D, -1, 0, fb_check=fb)
        assert outs[0].dtype == np.uint32
        _eq(outs[1], want["minC"], "d_min None after shifted calls: minC")
        _eq(outs[0], want["bestD"], "d_min None after shifted calls: disp")
        _eq(outs[0], R.calc_cost_sgm_linear(I1, I2, D, *R.rectified_maps(W, H, -1), 6, 64)[0], "d_min None: the unshifted restatement")
        if fb:
            assert outs[3].dtype == np.uint32
            _eq(outs[3], want["bestD2"], "d_min None after shifted calls: disp2 (512 << 8 where invalid)")
            _eq(outs[2], want["conf"], "d_min None after shifted calls: conf")


@pytest.mark.parametrize("W,H,D,direction,paths", [(61, 9, 32, -1, 4), (37, 12, 24, +1, 8), (5, 7, 16, -1, 4)])
def test_d_min_zero_through_range_equals_the_old_entry_point(gpu_lib, W, H, D, direction, paths):
    I1, I2 = synth.image_pair(W, H, D, seed=W)
    old = fsgm_amd.stereo_sgm(I1, I2, D, paths=paths, direction=direction, fb_check=1)
    new = fsgm_amd.stereo_sgm(I1, I2, D, paths=paths, direction=direction, fb_check=1, d_min=0)
    assert [a.dtype for a in old] == [np.uint32, np.uint32, np.uint8, np.uint32]
    assert [a.dtype for a in new] == [np.int32, np.uint32, np.uint8, np.int32]     # the dtype follows the argument, not its value
    _eq(new[0], old[0].astype(np.int64), "disp")
    _eq(new[1], old[1], "minC")
    _eq(new[2], old[2], "conf")
    _eq(new[3], np.where(old[3] == OLD_MARKER, SR.INT32_MIN, old[3].astype(np.int64)), "disp2")
    assert (old[3] == OLD_MARKER).any()
