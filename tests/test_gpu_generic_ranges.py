"""GPU tests of the generic line kernel and the generic WTA (agg_generic_kernel, epi_lines.hip; wta_generic_kernel, epi_wta.hip) at the
disparity ranges they serve from 144 to FSGM_GENERIC_MAX_D = 1024: 3 to 16 strides of 64 lanes, the d == D - 1 end in a late
stride, a ragged last stride (257, 1023), the LDS rows filled to their last byte (1024), winners beyond the 8 bits the packed WTA
keeps for d, and the cost stage's two-kernel form beyond 256.  Every compared output is an integer array compared for equality
with the CPU oracle (pinned to the reference's compiled code at 144, 240, 300, 512, 1023 and 1024 disparities in
tests/test_generic_ranges_cpu.py) or with the numpy restatements the adaptive-P2 and stereo tests use.  Every case names the
pipeline it expects.  Where a test is about the upper range it asserts, from the oracle's results alone, that the winners do
reach it.

The two shapes, 37x21 and 13x26: a workgroup holds four lines, a line per wave, against 21, 37, 13 or 26 lines -- several
workgroups and a partial one --, diagonals that re-enter at both borders with W > H and W < H, and the mirrored pass.
The torch op: tests/test_gpu_generic_ranges_torch.py."""
import functools

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, synth
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA
from fsgm_amd.epi import auto_pipeline
from tests import adaptive_p2_restatement as A
from tests import mexharness as mh
from tests import stereo_restatement as R
from tests.test_generic_ranges_cpu import LARGE, epi_case

pytestmark = pytest.mark.gpu

RANGES = (144, 176, 208, 240, 257, 300, 511, 1000, 1023, 1024)
SHAPES = ((37, 21), (13, 26))
NOWRAP, WRAP = "nowrap", "wrap"
PENALTIES = {NOWRAP: (6, 64), WRAP: (100, 200)}
GENERIC = "generic"
TIE_ROWS = (16, 18)                                              # costs equal for every d; costs of period 64 in d


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def _planted(W, H, D):
    """((y, x), d): the one d whose cost is 0 at that pixel, every other at the volume's maximum.  best == D - 1 at an interior
    pixel (the parabola reads the next pixel's d = 0) and at the frame's last pixel (the word past the array: 0), best == 1 and 0
    (never refined), and where D holds them the ends of a stride of 64 lanes and of the packed WTA's 8 bits.  Among noise such a
    pixel pulls the winner towards d, no more: with hundreds of candidates some path sums end lower elsewhere.  The winners
    that are certain are test_winner_at_every_stride_and_bit_end's."""
    spots = [((2, 3), D - 1), ((4, 5), 1), ((6, 7), 0), ((H - 1, W - 1), D - 1)]
    spots += [(yx, d) for yx, d in (((8, 2), 63), ((8, 6), 64), ((10, 3), 255), ((10, 8), 256), ((12, 5), 257)) if d < D - 1]
    return spots


@functools.lru_cache(maxsize=None)
def _volume(W, H, D, kind):
    """costs up to 24 for the no-wrap penalties, over the whole byte range for the wrapping ones (every mod-256 narrowing
    taken), with the planted pixels and the two tie rows.  At 300 disparities a uniform draw leaves the upper 44 candidates a
    seventh of the wins: there the costs below d = 256 are raised to a quarter of the range at least, and the upper candidates
    take the quarter of the pixels that test_aggregation_and_wta_match_the_oracle asks for (0.28 to 0.43 under the wrapping
    penalties, 0.98 and more under the others)."""
    hi = 24 if kind == NOWRAP else 255
    Cv = synth.cost_volume(W, H, D, seed=W * 7 + D, cmax=24) if kind == NOWRAP else synth.uniform_u8(W * 7 + D, (H, W, D))
    if D >= 300 and 4 * (D - 256) < D:
        Cv[:, :, :256] = np.maximum(Cv[:, :, :256], hi // 4)
    Cv[TIE_ROWS[0]] = hi // 3
    Cv[TIE_ROWS[1]] = Cv[TIE_ROWS[1]][:, np.arange(D) % 64]
    for (y, x), d in _planted(W, H, D):
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
def _sums(W, H, D, kind, paths):
    """the oracle's S for _volume, computed once and shared"""
    from oracle import pyoracle
    S = pyoracle.epi_aggregate(_volume(W, H, D, kind), *PENALTIES[kind], paths)
    S.setflags(write=False)
    return S


def _first_minimum(S, W, H, D):
    """numpy's statement of :259-277: the first d of the smallest sum"""
    return S[:-1].reshape(H, W, D).argmin(axis=2)


# ------------------------------------------------------------------------------------------ aggregation and WTA from volumes
@pytest.mark.parametrize("subpixel,vz", ((1, 1), (0, 0), (1, 0), (0, 1)))
@pytest.mark.parametrize("kind", (NOWRAP, WRAP))
@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("D", RANGES)
def test_aggregation_and_wta_match_the_oracle(gpu_lib, oracle, D, W, H, paths, kind, subpixel, vz):
    S, off = _sums(W, H, D, kind, paths), _offsets(W, H)
    idx, _ = oracle.epi_wta(S, W, H, D, 0)
    _eq(idx, _first_minimum(S, W, H, D), "the oracle's winner is the first minimum")
    if D >= 300:
        share = float((idx >= 256).mean())
        print(f"{W}x{H}x{D} {kind} {paths} paths: share of winners >= 256 = {share:.3f}")
        assert share >= 0.25, share
    bd, mc = oracle.epi_wta(S, W, H, D, subpixel)
    if vz:
        bd = oracle.epi_vz_to_disp(bd, off, 0.3, D + 1)
    with EpiPlan(W, H, D, 1, paths=paths, subpixel=subpixel, vz_to_disp=vz) as plan:
        plan.set_penalties(*PENALTIES[kind], 0.3)
        plan.upload_cost(0, _volume(W, H, D, kind))
        plan.upload_offset(0, off)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == GENERIC
        gbd, gmc = plan.download(0)
        gS = plan.download_sum(0)
    _eq(gS, S[:-1].reshape(H, W, D), "S")
    _eq(gmc, mc, "minC")
    _eq(gbd, bd, "bestD")


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("D", RANGES)
def test_winner_at_every_stride_and_bit_end(gpu_lib, oracle, D, paths):
    """Every pixel's cost is 0 at one d and 12 to 24 elsewhere: on every path that d stays at 0 and the minimum with it, every
    other d at 12 or more, so it wins at every pixel, the frame's last included.  d = 0, 1 (never refined), the ends of the
    first stride of 64 lanes, the ends of 8 bits, and D - 2, D - 1 in the last, possibly ragged, stride."""
    W, H = 7, 6
    noise = 12 + synth.uniform_u8(D + paths, (H, W, D), hi=12)
    with EpiPlan(W, H, D, 1, paths=paths, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64, 0.3)
        for t in sorted({t for t in (0, 1, 2, 63, 64, 65, 255, 256, 257, D - 2, D - 1) if t < D}):
            Cv = noise.copy()
            Cv[:, :, t] = 0
            S = oracle.epi_aggregate(Cv, 6, 64, paths)
            assert (oracle.epi_wta(S, W, H, D, 0)[0] == t).all(), t          # the oracle's winner is t at every pixel
            bd, mc = oracle.epi_wta(S, W, H, D, 1)
            assert not mc.any() and (np.abs(bd.astype(np.int64) - 256 * t) <= 128).all(), t     # the parabola: half a step at most
            plan.upload_cost(0, Cv)
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            assert plan.kernel_name == GENERIC
            gbd, gmc = plan.download(0)
            _eq(gmc, mc, f"minC, winner {t}")
            _eq(gbd, bd, f"bestD, winner {t}")


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("D,period", ((300, 64), (1024, 64), (1023, 1)))
def test_first_minimum_wins_across_strides_and_lanes(gpu_lib, oracle, D, period, paths):
    """Every pixel's costs repeat with the period in d (period 1: a flat volume), so the sums tie between strides, or between
    all lanes and strides: the winner is the first of them."""
    W, H = 13, 26
    base = synth.cost_volume(W, H, period, seed=D + period, cmax=24)
    Cv = np.ascontiguousarray(base[:, :, np.arange(D) % period])
    S = oracle.epi_aggregate(Cv, 6, 64, paths)
    Sv = S[:-1].reshape(H, W, D)
    tied = ((Sv == Sv.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean()
    assert tied >= 0.5, tied                                     # the oracle's sums do tie on most pixels
    bd, mc = oracle.epi_wta(S, W, H, D, 1)
    _eq(oracle.epi_wta(S, W, H, D, 0)[0], _first_minimum(S, W, H, D), "the oracle's winner is the first minimum")
    with EpiPlan(W, H, D, 1, paths=paths, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload_cost(0, Cv)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == GENERIC
        gbd, gmc = plan.download(0)
        gS = plan.download_sum(0)
    _eq(gS, Sv, "S")
    _eq(gmc, mc, "minC")
    _eq(gbd, bd, "bestD")


@pytest.mark.parametrize("D,paths", ((300, 8), (1024, 4)))
def test_batch_of_three_distinct_volumes_through_one_plan(gpu_lib, oracle, D, paths):
    """a wrong frame or direction stride of the path volumes shows"""
    W, H = 37, 21
    vols = [synth.cost_volume(W, H, D, seed=s, cmax=24) for s in (3, 4, 5)]
    offs = [synth.epi_maps(W, H, "general", seed=s)[2] for s in (3, 4, 5)]
    with EpiPlan(W, H, D, 3, paths=paths) as plan:
        plan.set_penalties(6, 64, 0.3)
        for f in range(3):
            plan.upload_cost(f, vols[f])
            plan.upload_offset(f, offs[f])
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == GENERIC
        got = [plan.download(f) + (plan.download_sum(f),) for f in range(3)]
    want = []
    for f in range(3):
        S = oracle.epi_aggregate(vols[f], 6, 64, paths)
        bd, mc = oracle.epi_wta(S, W, H, D, 1)
        want.append(mc)
        _eq(got[f][2], S[:-1].reshape(H, W, D), f"S of frame {f}")
        _eq(got[f][1], mc, f"minC of frame {f}")
        _eq(got[f][0], oracle.epi_vz_to_disp(bd, offs[f], 0.3, D + 1), f"bestD of frame {f}")
    assert (want[0] != want[1]).any() and (want[1] != want[2]).any()


# ------------------------------------------------------------------------------------------ adaptive P2
@pytest.mark.parametrize("kind", (NOWRAP, WRAP))
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("D", (144, 300, 1024))                  # 3, 5 and 16 strides
def test_adaptive_p2_matches_the_restatement(gpu_lib, oracle, D, W, H, kind):
    P1, P2 = PENALTIES[kind]
    Cv = _volume(W, H, D, kind)
    I1 = synth.uniform_u8(W + D, (H, W))                         # raw noise: most steps cross an intensity edge
    Sa = A.aggregate(Cv, I1, P1, P2, 8, 1)
    want = oracle.epi_wta(Sa, W, H, D, 1)
    with EpiPlan(W, H, D, 1, paths=8, vz_to_disp=0, adaptive_p2=1) as plan:
        plan.set_penalties(P1, P2, 0.3)
        plan.upload_cost(0, Cv)
        plan.upload_images(0, I1, I1)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == GENERIC
        got = plan.download(0) + (plan.download_sum(0),)
        plan.set_adaptive_p2(0)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == GENERIC
        plain = plan.download(0) + (plan.download_sum(0),)
    _eq(got[2], Sa[:-1].reshape(H, W, D), "S")
    _eq(got[1], want[1], "minC")
    _eq(got[0], want[0], "bestD")
    S = _sums(W, H, D, kind, 8)
    pbd, pmc = oracle.epi_wta(S, W, H, D, 1)
    _eq(plain[2], S[:-1].reshape(H, W, D), "S, adaptive off")
    _eq(plain[1], pmc, "minC, adaptive off")
    _eq(plain[0], pbd, "bestD, adaptive off")
    assert (plain[1] != got[1]).any()                            # the switch does something on this frame


# ------------------------------------------------------------------------------------------ forced modes
@pytest.mark.parametrize("D", (240, 512))
def test_forced_fused_modes_leave_the_generic_kernels_in_place(gpu_lib, oracle, D):
    W, H = 37, 21
    Cv = synth.cost_volume(W, H, D, seed=D, cmax=24)
    bd, mc = oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, 8), W, H, D, 1)
    with EpiPlan(W, H, D, 1, paths=8, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload_cost(0, Cv)
        for mode in (2, 3, 4, 5, 6):
            plan.set_agg_mode(mode)
            assert plan.kernel_name == GENERIC, mode
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            assert plan.kernel_name == GENERIC, mode
            gbd, gmc = plan.download(0)
            _eq(gmc, mc, f"minC, mode {mode}")
            _eq(gbd, bd, f"bestD, mode {mode}")


# ------------------------------------------------------------------------------------------ whole calls from images
# the frames pinned to the reference in tests/test_generic_ranges_cpu.py; 257 and 260 at 33x21: epi_rawcost_kernel<false> with
# box5x5_kernel and epi_rawcost_kernel<true> with box5x5_sliding_kernel (300 takes the latter pair too; 144, 512 and 1024
# epi_rawcost_px_kernel with box5x5_sliding16_kernel; 1023 the first pair)
WHOLE = LARGE + [(23, 9, 144, "general", 6, 64), (33, 21, 257, "general", 6, 64), (33, 21, 260, "general", 6, 64)]


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("W,H,D,kind,P1,P2", WHOLE)
def test_calc_cost_sgm_from_images(gpu_lib, oracle, W, H, D, kind, P1, P2, paths):
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = epi_case(W, H, D, kind, P1, P2)
    bd, mc, Cv, S = oracle.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths, want_volumes=True)
    assert auto_pipeline(W, H, D, 1, paths, P1, P2) == GENERIC   # the one-shot call's plan is chosen by this function
    gbd, gmc, gC, gS = fsgm_amd.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=paths, return_volumes=True)
    _eq(gC, Cv, "C")
    _eq(gS, S, "S")
    _eq(gmc, mc, "minC")
    _eq(gbd, bd, "bestD")


# frames chosen on the CPU: the oracle's winners are >= 256 on 0.61 and 0.37 of the pixels, up to 507 and 509
@pytest.mark.parametrize("kind,paths", (("radial", 8), ("general", 4)))
def test_forward_backward_check_at_its_largest_range(gpu_lib, oracle, kind, paths):
    """dMax = 511: bestD reaches 510 * 256, just below the check's INVALID = 512 << 8."""
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = epi_case(40, 26, 511, kind, 6, 64)
    H, W = I1.shape
    S = oracle.epi_aggregate(oracle.epi_cost(I1, I2, D, vMax, pd0, nd, off), P1, P2, paths)
    idx = oracle.epi_wta(S, W, H, D, 0)[0]
    share = float((idx >= 256).mean())
    print(f"{W}x{H}x{D} {kind}: share of winners >= 256 = {share:.3f}, largest {int(idx.max())}")
    assert share >= 0.15, share
    bd_idx, mc = oracle.epi_wta(S, W, H, D, 1)
    assert bd_idx.max() < 512 << 8
    conf, d2 = oracle.epi_fb_check(bd_idx, pd0, nd, off, vMax, D + 1)
    assert (conf[idx >= 256] == 1).any() and (conf[idx >= 256] == 0).any()    # large winners pass the check, and fail it
    assert (d2[d2 != (512 << 8)] >= 256 << 8).any()              # a large index went through the scatter
    assert auto_pipeline(W, H, D, 1, paths, P1, P2) == GENERIC
    gbd, gmc, gconf, gd2 = fsgm_amd.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=paths, fb_check=1)
    _eq(gmc, mc, "minC")
    _eq(gbd, oracle.epi_vz_to_disp(bd_idx, off, vMax, D + 1), "bestD")
    _eq(gd2, d2, "bestD2")
    _eq(gconf, conf, "conf")


@pytest.mark.parametrize("paths,sub", ((4, 1), (8, 0)))
def test_linear_build_matches_the_restatement(gpu_lib, oracle, paths, sub):
    W, H, D = 97, 13, 300
    I1, I2 = synth.image_pair(W, H, D, seed=12)
    pd0, nd, _ = synth.epi_maps(W, H, "general", seed=3)
    wbd, wmc, wC = R.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64, paths=paths, subpixel=sub, want_cost=True)
    assert auto_pipeline(W, H, D, 1, paths, 6, 64) == GENERIC
    bd, mc, Cv, _ = fsgm_amd.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64, paths=paths, subpixel=sub, return_volumes=True)
    _eq(Cv, wC, "C")
    _eq(mc, wmc, "minC")
    _eq(bd, wbd, "bestD")


# ------------------------------------------------------------------------------------------ rectified stereo
# 40x12: dMax > W, every far column clamps (stereo_rawcost_kernel); 330x6: dMax < W
@pytest.mark.parametrize("W,H,paths,direction,fb", [(40, 12, 4, -1, 0), (40, 12, 8, +1, 1), (330, 6, 8, -1, 1), (330, 6, 4, +1, 0)])
def test_stereo_sgm_matches_the_restatement(gpu_lib, oracle, W, H, paths, direction, fb):
    D = 300
    L, Rt = synth.image_pair(W, H, 16 if W < D else D, seed=W + paths)
    if direction > 0:
        L, Rt = Rt, L
    Cv = R.box_mean(R.rectified_raw_cost(L, Rt, D, direction))
    wbd, wmc = oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, paths), W, H, D, 1)
    assert auto_pipeline(W, H, D, 1, paths, 6, 64) == GENERIC
    got = fsgm_amd.stereo_sgm(L, Rt, D) if (paths, direction, fb) == (4, -1, 0) else \
        fsgm_amd.stereo_sgm(L, Rt, D, paths=paths, direction=direction, fb_check=fb)
    _eq(got[1], wmc, "minC")
    _eq(got[0], wbd, "disp")
    if fb:
        wconf, wd2 = R.linear_fb_check(wbd, *R.rectified_maps(W, H, direction))
        _eq(got[3], wd2, "disp2")
        _eq(got[2], wconf, "conf")


# ------------------------------------------------------------------------------------------ MEX gateway
def test_mex_gateway(gpu_lib, oracle):
    W, H = 23, 9
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = epi_case(W, H, 144, "general", 6, 64)
    bd, mc = oracle.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, 4)
    assert auto_pipeline(W, H, D, 1, 4, P1, P2) == GENERIC
    outs, _ = mh.call("calc_cost_sgm", 2, I1, I2, D, vMax, pd0, nd, off, P1, P2)
    _eq(outs[1], mc, "minC")
    _eq(outs[0], bd, "bestD")
