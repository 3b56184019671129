"""GPU tests of the runner-up cost of the 2-D matcher and of sgm(C) on caller-supplied 1-D volumes, and of the uniqueness filter on
flows.  The expected minC2 is always the numpy restatement (tests/runner_up2d_restatement.py, tests/runner_up_restatement.py)
applied to the ORACLE's S -- the oracle pinned to the reference's compiled code, as tests/test_gpu_sgm2d.py uses it -- and the
library's S must equal that S; bestD, minC and mvSub must equal those of the same call without runner_up.

Frames are 13x7 and 21x10: 91 and 210 pixels are no multiples of 16, so the row-packed WTA's last block has idle pixel slots.
Windows are written Sx x Sy; NW = ceil(Sy / 4) is the row-packed kernels' dwords per candidate row.

Which WTA kernel a case runs is launch_pyd_wta's choice (pyd_rows_wta_ok), apart from the aggregation that last_kernel() names:
windows up to 11x11 whose path weights sum to at most 257 take pyd_rows_wta_kernel<NW, true> -- under wrapping penalties too --
and everything else pyd_wta_kernel<true, .>, which keeps its sums up to 256 candidates (<true, 4>) and sums again above
(<true, 0>).  sgm2d_batch has totalPass <= 2, so through it the generic WTA runs for windows above 11x11 only; the PydPlan tests
at totalPass 64 / 65 reach it at 3x3 and 9x9, and the row-packed one at the top of its u16 sums."""
import ctypes as C
import functools

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import synth, sgm2d_batch, sgm_batch, calc_pyd_cost_sgm, calc_pyd_cost_sgm_batch, PydPlan
from fsgm_amd import _lib
from fsgm_amd._lib import FsgmError
from fsgm_amd.sgm2d import last_kernel
from oracle import pyoracle
from tests import runner_up_restatement as RU
from tests import runner_up2d_restatement as RU2

pytestmark = pytest.mark.gpu
NONE = RU.NO_RUNNER_UP
INVALID, UNSUPPORTED = 1, 4
FRAMES = [(13, 7), (21, 10)]
LINE_KERNELS = ("packed16/nowrap", "packed16/wrap", "generic")


def _volumes(W, H, D, n, seed, cmax):
    return np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])


_INPUTS = {}


@functools.lru_cache(maxsize=None)
def _oracle_cached(key, rX, rY, P1, P2, diag, passes):
    vols = _INPUTS[key]
    n, H, W, D = vols.shape
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    out = []
    for f in range(n):
        S = pyoracle.pyd_aggregate(np.zeros((H, W), np.uint8), vols[f], np.zeros((2, H, W)), Sx, Sy, P1, P2, diag, passes, 0)
        out.append(pyoracle.pyd_wta(S, Sx, Sy, 1) + (S,))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def _want(vols, rX, rY, P1, P2, diag=1, passes=2):
    """(bestD, minC, mvSub, S, minC2): the oracle's, once per distinct input, and the restatement on its S"""
    key = (vols.shape, hash(vols.tobytes()))
    _INPUTS.setdefault(key, vols)
    bd, mc, ms, S = _oracle_cached(key, rX, rY, P1, P2, diag, passes)
    b2, c2, m2 = RU2.runner_up2d(S, 2 * rX + 1, 2 * rY + 1)
    np.testing.assert_array_equal(b2, bd)                        # the restatement's WTA is the oracle's
    np.testing.assert_array_equal(c2, mc)
    return bd, mc, ms, S, m2


def _check(vols, rX, rY, P1, P2, bound, diag=1, passes=2):
    """the plain call, the runner-up call and the oracle; returns (expected minC2, the kernel the runner-up call ran)"""
    bd, mc, ms, S, m2 = _want(vols, rX, rY, P1, P2, diag, passes)
    kw = dict(layout="hwd", cost_bound=bound, diagonal=diag, total_pass=passes, return_sum=True)
    plain = sgm2d_batch(vols, rX, rY, P1, P2, **kw)
    k_plain = last_kernel()
    gbd, gmc, gm2, gms, gS = sgm2d_batch(vols, rX, rY, P1, P2, runner_up=True, **kw)
    assert last_kernel() == k_plain
    np.testing.assert_array_equal(gS, S, err_msg="S against the oracle")
    for g, p, w, name in zip((gbd, gmc, gms, gS), plain, (bd, mc, ms, S), ("bestD", "minC", "mvSub", "S")):
        np.testing.assert_array_equal(g, p, err_msg=f"{name} against the call without runner_up")
        np.testing.assert_array_equal(g, w, err_msg=f"{name} against the oracle")
    assert gm2.dtype == np.uint32
    np.testing.assert_array_equal(gm2, m2, err_msg="minC2")
    return m2, k_plain


@pytest.fixture(scope="module")
def rows_available(gpu_lib):
    """whether plans on this device hold the row-packed kernels' descriptors (tests/test_gpu_sgm2d.py: the device's self-test)"""
    sgm2d_batch(np.zeros((9, 2, 3), np.uint8), 1, 1, 6, 32, layout="dhw", cost_bound=24)
    return last_kernel().startswith("rows")


# ---------------------------------------------------------------------------------------------- row-packed kernel, every NW
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("Sx,Sy", [(1, 1), (3, 3), (3, 1), (1, 3), (5, 3), (7, 5), (9, 9), (3, 11), (11, 11)])
def test_row_packed_kernel(gpu_lib, oracle, rows_available, Sx, Sy, W, H, n):
    rX, rY = Sx // 2, Sy // 2
    vols = _volumes(W, H, Sx * Sy, n, seed=Sx + 3 * Sy + W, cmax=24)
    m2, kernel = _check(vols, rX, rY, 6, 32, 24)
    if rows_available:
        assert kernel.startswith("rows")
    if (Sx, Sy) == (1, 1):
        assert (m2 == NONE).all()
    elif Sx <= 3 and Sy <= 3:                                    # empty where the best is in the middle of every side of 3
        assert (m2 == NONE).any() and (m2 != NONE).any()
    else:
        assert (m2 != NONE).all()


# ---------------------------------------------------------------------------------------------- wrapping penalties, generic kernel
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("Sx,Sy", [(3, 3), (9, 9)])
def test_wrapping_aggregation_row_packed_wta(gpu_lib, oracle, Sx, Sy, W, H, n):
    """P1 = 100, P2 = 200: the generic wrapping AGGREGATION, whose sums (the S tap's, wrapped) the WTA minimises; the WTA itself is
    still the row-packed one at these windows and two passes (pyd_rows_wta_ok)"""
    vols = _volumes(W, H, Sx * Sy, n, seed=Sx + W, cmax=255)
    _, kernel = _check(vols, Sx // 2, Sy // 2, 100, 200, 255)
    assert kernel == "generic/wrap"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W,H", FRAMES)
def test_generic_kernel_13x13(gpu_lib, oracle, W, H, n):
    """above the row-packed limit: pyd_wta_kernel<true, 4>, 169 candidates, three of its four kept sums a lane, the last partial"""
    m2, kernel = _check(_volumes(W, H, 169, n, seed=W, cmax=24), 6, 6, 6, 32, 24)
    assert kernel == "generic" and (m2 != NONE).all()


@pytest.mark.parametrize("n", [1, 3])
def test_generic_kernel_1023_candidates(gpu_lib, oracle, n):
    """pyd_wta_kernel<true, 0>: the second pass sums the path bytes again, 16 strides of 64"""
    m2, kernel = _check(_volumes(13, 7, 1023, n, seed=5, cmax=24), 15, 16, 6, 32, 24)
    assert kernel == "generic" and (m2 != NONE).all()


# ---------------------------------------------------------------------------------------------- adversarial volumes
@pytest.mark.parametrize("Sx,Sy", [(3, 3), (5, 3), (9, 9), (13, 13)])
def test_constant_volume(gpu_lib, oracle, Sx, Sy):
    """all candidates tie: best = 0, and minC2 == minC wherever the set is not empty (3x3 with the best in a corner: it is not)"""
    W, H = 21, 10
    vols = np.full((3, H, W, Sx * Sy), 9, np.uint8)
    bd, mc, _, _, m2 = _want(vols, Sx // 2, Sy // 2, 6, 32)
    assert not bd.any()
    np.testing.assert_array_equal(m2, mc)
    _check(vols, Sx // 2, Sy // 2, 6, 32, 24)


@pytest.mark.parametrize("Sx,Sy,P1,P2,bound", [(5, 3, 6, 32, 24), (9, 9, 6, 32, 24), (9, 9, 100, 200, 255), (13, 13, 6, 32, 24)])
def test_dense_ties(gpu_lib, oracle, Sx, Sy, P1, P2, bound):
    """costs from {0, 1, 2, 3}: the first-minimum rule decides where the mask lies"""
    W, H = 21, 10
    vols = np.random.default_rng(Sx * Sy).integers(0, 4, (3, H, W, Sx * Sy)).astype(np.uint8)
    bd, mc, _, S, m2 = _want(vols, Sx // 2, Sy // 2, P1, P2)
    assert ((S == mc[..., None]).sum(-1) > 1).any(), "no tied minimum in the expected sums"
    _check(vols, Sx // 2, Sy // 2, P1, P2, bound)


def _planted(W, H, Sx, Sy):
    """One frame per position of the minimum -- the window's four corners, four edge midpoints and centre -- each pixel the same
    vector: 0 at the position, 1 inside the excluded ring, 2 just outside it (Chebyshev distance 2), 20 elsewhere.  With
    P1 = P2 = 0 every path cost is the cost itself, so S = 8 C with two passes and diagonals."""
    cx, cy = Sx // 2, Sy // 2
    spots = [(0, 0), (0, Sy - 1), (Sx - 1, 0), (Sx - 1, Sy - 1), (0, cy), (Sx - 1, cy), (cx, 0), (cx, Sy - 1), (cx, cy)]
    vols = np.full((len(spots), H, W, Sx, Sy), 20, np.uint8)
    for f, (bx, by) in enumerate(spots):
        ring = [(x, y) for x in range(Sx) for y in range(Sy) if max(abs(x - bx), abs(y - by)) == 1]
        far = [(x, y) for x in range(Sx) for y in range(Sy) if max(abs(x - bx), abs(y - by)) == 2]
        vols[f, :, :, bx, by] = 0
        x, y = ring[f % len(ring)]
        vols[f, :, :, x, y] = 1
        x, y = far[(3 * f) % len(far)]
        vols[f, :, :, x, y] = 2
    return vols.reshape(len(spots), H, W, Sx * Sy), spots


@pytest.mark.parametrize("Sx,Sy", [(5, 5), (7, 5), (9, 9), (11, 11), (13, 13)])
def test_planted_minimum_second_in_the_ring_third_outside(gpu_lib, oracle, Sx, Sy):
    W, H = 13, 7
    vols, spots = _planted(W, H, Sx, Sy)
    bd, mc, _, S, m2 = _want(vols, Sx // 2, Sy // 2, 0, 0)
    np.testing.assert_array_equal(S, 8 * vols.astype(np.uint32))
    for f, (bx, by) in enumerate(spots):
        assert (bd[f] == bx * Sy + by).all() and (mc[f] == 0).all()
    assert (m2 == 16).all(), "the third-smallest cost, not the second"
    _check(vols, Sx // 2, Sy // 2, 0, 0, 24)


@pytest.mark.parametrize("P1,P2", [(0, 0), (6, 32)])
def test_sums_at_the_u16_ceiling(gpu_lib, oracle, P1, P2):
    """all bytes 255, two passes with diagonals, through sgm2d_batch: S = 2040 at most, the row-packed WTA under either penalty
    set (the aggregation is generic/wrap with (6, 32)).  The top of the u16 sums, 65280, needs totalPass 64:
    test_pyd_plan_around_the_u16_bound"""
    vols = np.full((1, 10, 21, 81), 255, np.uint8)
    bd, mc, _, S, m2 = _want(vols, 4, 4, P1, P2)
    if (P1, P2) == (0, 0):
        assert (S == 2040).all() and (m2 == 2040).all()
    _check(vols, 4, 4, P1, P2, 255)


def _rows_wta(Sx, Sy, diag, passes):
    """pyd_rows_wta_ok restated (tests/test_gpu_pyd_windows.py): rows layout, every weight a byte, the weighted sums a u16"""
    nd = 4 if diag else 2
    weights = ([1] * nd if passes >= 1 else []) + ([passes - 1] * nd if passes >= 2 else [])
    return Sx <= 11 and Sy <= 11 and all(w <= 255 for w in weights) and sum(weights) * 255 <= 65535


@pytest.mark.parametrize("passes", [64, 65])
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("Sx,Sy", [(3, 3), (9, 9)])
def test_pyd_plan_around_the_u16_bound(gpu_lib, oracle, Sx, Sy, W, H, passes):
    """totalPass 64 with diagonals: the last pass count whose weighted sums fit u16 -- pyd_rows_wta_kernel<NW, true> with sums up
    to 65280 = 0xFF00, where a u16 reduction or a u16 marker would confuse a sum with FSGM_NO_RUNNER_UP.  totalPass 65: the
    first that does not fit -- pyd_wta_kernel<true, 4> at 9 candidates (55 lanes of the wave without one, whose kept sum must
    stay the identity) and at 81 (a partial second stride).  P1 = P2 = 0, so every path cost is the cost itself; frame 0 is the
    constant-255 volume, frame 1 costs 250..255."""
    rX, rY, D = Sx // 2, Sy // 2, Sx * Sy
    assert _rows_wta(Sx, Sy, 1, passes) == (passes == 64)
    I1, I2 = synth.image_pair(W, H, 8, seed=17)
    mv = synth.hint_map(W + 2, H + 1, "general", seed=19, amp=3.0)
    vols = [np.full((H, W, D), 255, np.uint8), (250 + synth.uniform_u8(23, (H, W, D), hi=5)).astype(np.uint8)]
    assert vols[1].min() == 250 and vols[1].max() == 255
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2, batch=2) as plan:
        plan.set_params(0, 0, 1, passes, 0, 1)
        for f in range(2):
            plan.upload(f, I1, I2, mv)
            plan.upload_cost(f, vols[f])
        plan.run(_lib.STAGE_AGGREGATE | _lib.STAGE_WTA)
        plain = [plan.download(f) for f in range(2)]
        plan.set_runner_up(1)
        plan.run(_lib.STAGE_AGGREGATE | _lib.STAGE_WTA)
        for f in range(2):
            S = pyoracle.pyd_aggregate(I1, vols[f], mv, Sx, Sy, 0, 0, 1, passes, 0)
            np.testing.assert_array_equal(S, 4 * passes * vols[f].astype(np.uint32))     # weights 1 and totalPass - 1
            bd, mc, ms = pyoracle.pyd_wta(S, Sx, Sy, 1)
            b2, c2, m2 = RU2.runner_up2d(S, Sx, Sy)
            np.testing.assert_array_equal(b2, bd)
            np.testing.assert_array_equal(plan.download_sum(f), S, err_msg="S against the oracle")
            for g, p, w, name in zip(plan.download(f), plain[f], (bd, mc, ms), ("bestD", "minC", "mvSub")):
                np.testing.assert_array_equal(g, p, err_msg=f"{name} against the run without the switch")
                np.testing.assert_array_equal(g, w, err_msg=f"{name} against the oracle")
            got = plan.download_runner_up(f)
            np.testing.assert_array_equal(got, m2, err_msg=f"minC2, frame {f}")
            if f == 0:                                           # all candidates tie at the largest sum: best 0, a corner
                assert (S == 1020 * passes).all() and (got == 1020 * passes).all()
                assert S[0, 0, 0] == (65280 if passes == 64 else 66300)
            elif (Sx, Sy) == (3, 3):
                assert (got == NONE).any() and (got != NONE).any()
            else:
                assert (got != NONE).all() and (got > 60000).all()


# ---------------------------------------------------------------------------------------------- the image-pair form
def _pair(seed=4):
    W, H = 21, 10
    I1, I2 = synth.image_pair(W, H, 8, seed=seed)
    mv = np.ascontiguousarray(np.round(synth.hint_map(W, H, "int", seed=seed + 2, amp=3.0)))
    assert mv.any() and (mv == np.round(mv)).all()
    return I1, I2, mv


@pytest.mark.parametrize("adaptive", [0, 1])
def test_calc_pyd_cost_sgm_runner_up(gpu_lib, oracle, adaptive):
    I1, I2, mv = _pair()
    I1 = (I1.astype(np.int32) * 3 % 256).astype(np.uint8)            # larger gradients: the adaptive branch is taken
    bd, mc, ms, Cv, S = pyoracle.calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, adaptive, want_volumes=True)
    m2 = RU2.runner_up2d(S, 9, 9)[2]
    plain = calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, adaptive, return_volumes=True)
    got = calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, adaptive, return_volumes=True, runner_up=True)
    assert len(got) == 6
    for g, p, w, name in zip(got[:5], plain, (bd, mc, ms, Cv, S), ("bestD", "minC", "mvSub", "C", "S")):
        np.testing.assert_array_equal(g, p, err_msg=f"{name} against the call without runner_up")
        np.testing.assert_array_equal(g, w, err_msg=f"{name} against the oracle")
    np.testing.assert_array_equal(got[5], m2)
    short = calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, adaptive, runner_up=True)
    assert len(short) == 4
    np.testing.assert_array_equal(short[3], m2)
    frames = [(I1, I2, mv)] * 3
    for r in calc_pyd_cost_sgm_batch(frames, 4, 4, 2, 1, 6, 32, 1, 2, adaptive, runner_up=True):
        assert len(r) == 4
        np.testing.assert_array_equal(r[0], bd)
        np.testing.assert_array_equal(r[3], m2)


def test_pyd_plan_switch(gpu_lib, oracle):
    I1, I2, mv = _pair(seed=9)
    W, H = 21, 10
    S = pyoracle.calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, 0, want_volumes=True)[4]
    m2 = RU2.runner_up2d(S, 9, 9)[2]
    with PydPlan(W, H, W, H, 4, 4, 2, batch=2) as plan:
        plan.set_params(6, 32, 1, 2, 0, 1)
        for f in range(2):
            plan.upload(f, I1, I2, mv)
        with pytest.raises(FsgmError) as e:
            plan.download_runner_up(0)
        assert e.value.status == INVALID
        plan.set_runner_up(1)
        assert (plan.download_runner_up(1) == NONE).all()        # all ones until a WTA has run
        plan.run()
        first = [plan.download(f) for f in range(2)]
        for f in range(2):
            np.testing.assert_array_equal(plan.download_runner_up(f), m2)
            np.testing.assert_array_equal(plan.download_sum(f), S)
        plan.set_runner_up(0)
        plan.run()
        with pytest.raises(FsgmError) as e:
            plan.download_runner_up(0)
        assert e.value.status == INVALID and "switch is off" in str(e.value)
        for f in range(2):
            for a, b in zip(plan.download(f), first[f]):
                np.testing.assert_array_equal(a, b)
        plan.set_runner_up(1)
        plan.run()
        np.testing.assert_array_equal(plan.download_runner_up(0), m2)
        for bad in (2, -1):
            with pytest.raises(FsgmError) as e:
                plan.set_runner_up(bad)
            assert e.value.status == INVALID


# ---------------------------------------------------------------------------------------------- cached plans
def test_cached_plans_are_not_shared(gpu_lib, oracle):
    W, H = 21, 10
    vols = _volumes(W, H, 81, 3, seed=77, cmax=24)
    kw = dict(layout="hwd", cost_bound=24, return_flow=True, return_sum=True)
    before = sgm2d_batch(vols, 4, 4, **kw)
    k_before = last_kernel()
    ru = sgm2d_batch(vols, 4, 4, runner_up=True, **kw)
    np.testing.assert_array_equal(ru[2], _want(vols, 4, 4, 6, 32)[4])
    after = sgm2d_batch(vols, 4, 4, **kw)
    assert last_kernel() == k_before
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    I1, I2, mv = _pair(seed=12)
    before = calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, 0)
    calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, 0, runner_up=True)
    for a, b in zip(before, calc_pyd_cost_sgm(I1, I2, mv, 4, 4, 2, 1, 6, 32, 1, 2, 0)):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------- sgm(C), 1-D
_sgm_last_kernel = __import__("importlib").import_module("fsgm_amd.sgm").last_kernel


@functools.lru_cache(maxsize=None)
def _sgm_case(D, n):
    W, H = 24, 9
    vols = _volumes(W, H, D, n, seed=D + n, cmax=24)
    S = np.stack([np.asarray(pyoracle.epi_aggregate(v, 7, 100, 4))[:H * W * D].reshape(H, W, D) for v in vols])
    return vols, S, RU.runner_up(S)


@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("n", [1, 40])
@pytest.mark.parametrize("D", [2, 3, 16, 48, 144])
def test_sgm_batch_runner_up(gpu_lib, oracle, D, n, layout):
    vols, S, (best, minC, minC2) = _sgm_case(D, n)
    src = vols if layout == "hwd" else np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    kw = dict(layout=layout, cost_bound=24, subpixel=0, return_sum=True)
    plain = sgm_batch(src, 7, 100, **kw)
    k_plain = _sgm_last_kernel()
    gbd, gmc, gm2, gS = sgm_batch(src, 7, 100, runner_up=True, **kw)
    assert _sgm_last_kernel() in LINE_KERNELS
    np.testing.assert_array_equal(gS, S, err_msg="S against the oracle")
    np.testing.assert_array_equal(gbd, best)                     # (subpixel 0: bestD is the index itself)
    np.testing.assert_array_equal(gmc, minC)
    np.testing.assert_array_equal(gm2, minC2)
    if D == 2:
        assert (minC2 == NONE).all()
    if D == 3:
        assert (minC2 == NONE).any() and (minC2 != NONE).any()
    for g, p in zip((gbd, gmc, gS), plain):
        np.testing.assert_array_equal(g, p)
    again = sgm_batch(src, 7, 100, **kw)
    assert _sgm_last_kernel() == k_plain                         # the plain call keeps its plan and pipeline
    for a, b in zip(again, plain):
        np.testing.assert_array_equal(a, b)


def test_sgm_batch_runner_up_refuses_forced_modes(gpu_lib):
    vols = _volumes(24, 9, 16, 1, seed=1, cmax=24)
    with pytest.raises(FsgmError) as e:
        sgm_batch(vols, 7, 100, agg_mode=4, runner_up=True)
    assert e.value.status == UNSUPPORTED
    assert len(sgm_batch(vols, 7, 100, agg_mode=1, runner_up=True)) == 3


# ---------------------------------------------------------------------------------------------- the filter
def _filter_inputs(n, H=10, W=21, seed=2):
    rng = np.random.default_rng(seed)
    minC = rng.integers(0, 2041, (n, H, W)).astype(np.uint32)
    minC2 = np.maximum(minC, rng.integers(0, 2300, (n, H, W))).astype(np.uint32)
    minC.flat[::11] = 0
    minC2.flat[::7] = NONE
    minC2.flat[3::13] = 0xFFFFFFFE                               # (u64)minC2 * 100 is far beyond 32 bits
    minC.flat[3::26] = 0xFFFFFFF0
    minC2.flat[5::17] = minC.flat[5::17]
    flow = rng.normal(0, 3, (n, 2, H, W))
    flow[:, 0].flat[::5] = np.nan                                # NaNs that are there already, in one plane or both
    flow[:, 1].flat[::10] = np.nan
    return flow, minC, minC2


@pytest.mark.parametrize("ratio", [0, 1, 15, 99, 100])
@pytest.mark.parametrize("n", [1, 3])
def test_filter_on_flows(gpu_lib, n, ratio):
    flow, minC, minC2 = _filter_inputs(n)
    rej = RU.uniqueness_reject(minC, minC2, ratio)
    want = RU2.uniqueness_filter_flow(flow, minC, minC2, ratio)
    out = fsgm_amd.uniqueness_filter(flow, minC, minC2, ratio, planes=2)
    assert out.shape == flow.shape and out.dtype == np.float64
    np.testing.assert_array_equal(out, want)                     # (NaN == NaN in assert_array_equal)
    for pl in range(2):
        assert np.isnan(out[:, pl][rej]).all()
        keep = ~rej & ~np.isnan(flow[:, pl])
        np.testing.assert_array_equal(out[:, pl][keep], flow[:, pl][keep])
        assert np.isnan(out[:, pl][np.isnan(flow[:, pl])]).all()
    if ratio in (15, 99):
        assert rej.any() and not rej.all()
    if ratio == 0:
        assert not rej.any()
    one = fsgm_amd.uniqueness_filter(flow[0], minC[0], minC2[0], ratio, planes=2)     # (2, H, W)
    np.testing.assert_array_equal(one, want[0])


@pytest.mark.parametrize("ratio", [0, 15, 100])
def test_filter_planes_1_is_the_existing_filter(gpu_lib, ratio):
    flow, minC, minC2 = _filter_inputs(3, seed=8)
    m = np.ascontiguousarray(flow[:, 0])
    old = fsgm_amd.uniqueness_filter(m, minC, minC2, ratio)
    new = fsgm_amd.uniqueness_filter(m, minC, minC2, ratio, planes=1)
    assert old.tobytes() == new.tobytes()
    out = np.empty_like(m)
    lib, p = _lib.load(), _lib.ptr
    assert lib.fsgm_uniqueness_filter_planes_host(3, p(m), p(minC), p(minC2), 21, 10, 1, ratio, p(out), 0) == 0
    assert out.tobytes() == old.tobytes()


def test_filter_in_place_and_overlap(gpu_lib):
    flow, minC, minC2 = _filter_inputs(2, seed=4)
    want = RU2.uniqueness_filter_flow(flow, minC, minC2, 15)
    lib, p = _lib.load(), _lib.ptr
    buf = np.zeros(flow.size + 4)
    work = buf[:flow.size].reshape(flow.shape)
    work[...] = flow
    assert lib.fsgm_uniqueness_filter_planes_host(2, p(work), p(minC), p(minC2), 21, 10, 2, 15, p(work), 0) == 0     # out == map
    np.testing.assert_array_equal(work, want)
    work[...] = flow
    shifted = C.c_void_p(buf.ctypes.data + 32)
    assert lib.fsgm_uniqueness_filter_planes_host(2, p(work), p(minC), p(minC2), 21, 10, 2, 15, shifted, 0) == INVALID
    assert "map itself" in lib.fsgm_last_error().decode()
    np.testing.assert_array_equal(work, flow)
