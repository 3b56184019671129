"""The calc_pyd_cost_sgm path at search windows from 13 candidates a side to the limits it accepts (sides up to 63, up to 1024
candidates; tests/test_gpu_pyd.py stops at 13x11), and the two kernel-selection rules beside them at their boundaries.

Everything is compared bit for bit with the CPU oracle, which tests/test_oracle_ref_parity.py pins to the reference's compiled
MEX code at these same windows, penalty sets and pass counts (tests/ref_cases.py: pyd_window_cases; the case lists are shared).
Frames are a few pixels: nothing in these kernels depends on the frame beyond its line counts (the generic aggregation kernel
advances 4 lines a workgroup: 1, 4, 5, 7, 9 and 13 lines occur).

The library does not report which 2-D kernel ran.  For the cost stage the tests ask fsgm_pyd_launch_lds (pyd.launch_lds), which
evaluates the launcher's own rule; for the aggregation and WTA rules they restate the rule from its inputs (_nowrap, _rows_wta).
The restated aggregation rule names the row-packed kernels for windows up to 11x11 on the assumption that the plan's once-a-device
self-test of the packed 3-input minima passed (fsgm_pyd_plan_create); where it did not, the plan has no descriptors, the generic
kernels run those cases too, and the comparison with the oracle holds all the same."""
import numpy as np
import pytest

from fsgm_amd import synth, PydPlan, calc_pyd_cost_sgm, pyramidal_sgm, pyd
from fsgm_amd._lib import STAGE_COST, STAGE_AGGREGATE, STAGE_WTA, STAGE_ALL
from tests import py_restatement as P
from tests import ref_cases as R

pytestmark = pytest.mark.gpu


def _nowrap(P1, P2, cmax):
    """pyd_enqueue's rule: no u8 narrowing changes a value; with the rows layout (windows up to 11x11) the row-packed
    aggregation kernels run, otherwise pyd_agg_kernel<false, .>; beyond it pyd_agg_kernel<true, .>."""
    return P1 >= 0 and P2 >= 0 and cmax + P2 + max(P1, P2) <= 255


def _rows_wta(Sx, Sy, diag, passes):
    """pyd_rows_wta_ok: rows layout, every weight a byte, and the weighted sum of u8 path costs a u16."""
    nd = 4 if diag else 2
    weights = ([1] * nd if passes >= 1 else []) + ([passes - 1] * nd if passes >= 2 else [])
    return Sx <= 11 and Sy <= 11 and all(w <= 255 for w in weights) and sum(weights) * 255 <= 65535


def _lanes(Sx, Sy):
    """candidates a lane of pyd_agg_kernel holds: its NCMAX is 2, 4 or 16"""
    nc = (Sx * Sy + 63) // 64
    return 2 if nc <= 2 else 4 if nc <= 4 else 16


def test_the_windows_are_the_ones_each_kernel_form_needs():
    sides = [(2 * rX + 1, 2 * rY + 1) for rX, rY in R.WINDOWS]
    assert sides == [(13, 9), (15, 17), (17, 15), (17, 17), (31, 33), (63, 15), (15, 63), (63, 1), (1, 63), (11, 13), (13, 11)]
    assert [_lanes(*s) for s in sides] == [2, 4, 4, 16, 16, 16, 16, 2, 2, 4, 4]
    assert 15 * 17 == 255 and 17 * 17 == 289 and 31 * 33 == 1023          # the top of 4 a lane, the bottom and the top of 16
    for rX, rY in R.WINDOWS:                                               # none takes the row-packed layout
        assert pyd.launch_lds(rX, rY, 2)["rows_agg_lds"] == 0 and pyd.launch_lds(rX, rY, 2)["cost_kernel"] == "patch"
    assert pyd.launch_lds(31, 7, 2)["agg_lds"] == 60448


def _frame(W, H, kind, seed, grad=3):
    I1, I2 = synth.image_pair(W, H, 16, seed=seed)
    if grad != 1:
        I1 = (I1.astype(np.int32) * grad % 256).astype(np.uint8)          # larger gradients: adaptive P2 branch taken
    return I1, I2, R.window_hints(W + 2, H + 1, kind, seed + 2, amp=4.0)


# ------------------------------------------------------------------------------------------------ cost stage
@pytest.mark.parametrize("W,H,rX,rY,rAgg,kind", R.window_cost_cases())
def test_cost_volume_bit_exact(gpu_lib, oracle, W, H, rX, rY, rAgg, kind):
    want_kernel = "candidate" if (rX, rY, rAgg) == R.COST_FALLBACK else "patch"
    info = pyd.launch_lds(rX, rY, rAgg)
    assert info["cost_kernel"] == want_kernel
    if (rX, rY, rAgg) == R.COST_PATCH_AT_BOUND:
        assert info["cost_lds"] == 49152
    I1, I2, mv = _frame(W, H, kind, W + rX, grad=1)
    want = oracle.pyd_cost(oracle.census(I1), oracle.census(I2), mv, rAgg, rX, rY)
    if kind == "outside":                                                  # every tap of every candidate adds the constant 5
        assert (want == 5).all()
    with PydPlan(W, H, W + 2, H + 1, rX, rY, rAgg) as plan:
        plan.upload(0, I1, I2, mv)
        plan.run(STAGE_COST)
        got = plan.download_cost(0)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ aggregation + WTA
def _run_uploaded(plan, f, I1, I2, mv, Cv):
    plan.upload(f, I1, I2, mv)
    plan.upload_cost(f, Cv)


def _compare(plan, f, oracle, I1, Cv, mv, Sx, Sy, P1, P2, diag, passes, adaptive, tag=""):
    S = oracle.pyd_aggregate(I1, Cv, mv, Sx, Sy, P1, P2, diag, passes, adaptive)
    bd, mc, ms = oracle.pyd_wta(S, Sx, Sy, 1)
    gS = plan.download_sum(f)
    gbd, gmc, gms = plan.download(f)
    np.testing.assert_array_equal(gS, S, err_msg=f"S {tag}")
    np.testing.assert_array_equal(gbd, bd, err_msg=f"bestD {tag}")
    np.testing.assert_array_equal(gmc, mc, err_msg=f"minC {tag}")
    np.testing.assert_array_equal(gms, ms, err_msg=f"mvSub {tag}")
    return S


@pytest.mark.parametrize("W,H,rX,rY,P1,P2,cmax,diag,passes,adaptive,kind", R.window_agg_cases(R.WINDOW_AGG_CROSS))
def test_aggregate_and_wta_bit_exact(gpu_lib, oracle, W, H, rX, rY, P1, P2, cmax, diag, passes, adaptive, kind):
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    I1, I2, mv = _frame(W, H, kind, 3 + rY)
    Cv = synth.cost_volume(W, H, Sx * Sy, seed=7 + rX, cmax=cmax)
    Cv[-1, -1, -1] = cmax
    assert Cv.max() == cmax and _nowrap(P1, P2, cmax) == (cmax == 24)      # pyd_agg_kernel<false, .> / <true, .>
    if kind == "jumpy":                        # every step of every path direction leaves the window in one axis at least
        m = mv[:, :H, :W]
        for a, b in ((m[:, :, 1:], m[:, :, :-1]), (m[:, 1:, :], m[:, :-1, :]), (m[:, 1:, 1:], m[:, :-1, :-1]), (m[:, 1:, :-1], m[:, :-1, 1:])):
            d = np.abs(a - b)                                              # along x, along y, (+1,+1), (-1,+1)
            assert ((d[0] > Sx + 3) | (d[1] > Sy + 3)).all()
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2) as plan:
        plan.set_params(P1, P2, diag, passes, adaptive, 1)
        _run_uploaded(plan, 0, I1, I2, mv, Cv)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        _compare(plan, 0, oracle, I1, Cv, mv, Sx, Sy, P1, P2, diag, passes, adaptive)


@pytest.mark.parametrize("P1,P2,cmax", R.WINDOW_PENALTIES)
@pytest.mark.parametrize("rX,rY", [(8, 8), (15, 16)])
def test_batch_of_three_frames(gpu_lib, oracle, rX, rY, P1, P2, cmax):
    """The frame strides of the volumes multiply by 289 or 1023 candidates."""
    W, H, Sx, Sy = 9, 5, 2 * rX + 1, 2 * rY + 1
    frames = [_frame(W, H, ("general", "int", "jumpy")[f], 20 + f) + (synth.cost_volume(W, H, Sx * Sy, seed=30 + f, cmax=cmax),) for f in range(3)]
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2, batch=3) as plan:
        plan.set_params(P1, P2, 1, 2, 1, 1)
        for f, (I1, I2, mv, Cv) in enumerate(frames):
            _run_uploaded(plan, f, I1, I2, mv, Cv)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        for f, (I1, I2, mv, Cv) in enumerate(frames):
            _compare(plan, f, oracle, I1, Cv, mv, Sx, Sy, P1, P2, 1, 2, 1, tag=f"frame {f}")


@pytest.mark.parametrize("W,H,rX,rY,rAgg,sub,P1,P2,diag,passes,adaptive,kind", R.window_whole_cases())
def test_whole_call(gpu_lib, oracle, W, H, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive, kind):
    I1, I2, mv = _frame(W, H, kind, 9 + rX)
    a = (rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive)
    want = oracle.calc_pyd_cost_sgm(I1, I2, mv, *a, want_volumes=True)
    got = calc_pyd_cost_sgm(I1, I2, mv, *a, return_volumes=True)
    for g, w, n in zip(got, want, ("bestD", "minC", "mvSub", "C", "S")):
        np.testing.assert_array_equal(g, w, err_msg=n)


def test_pyramidal_sgm_with_17x17_windows(gpu_lib, oracle):
    I0, I1 = synth.image_pair(24, 16, 12, seed=5)
    want_mv, want_minC, want_lv = oracle.pyramidal_sgm(I0, I1, 2, 6, 32, 2, 8, 8)
    mv, mvPyd, minC = pyramidal_sgm(I0, I1, 2, verSearchHalfWinSize=8, horSearchHalfWinSize=8)
    for l in (1, 0):
        np.testing.assert_array_equal(mvPyd[l], want_lv[l], err_msg=f"level {l + 1}")
    np.testing.assert_array_equal(mv, want_mv)
    np.testing.assert_array_equal(minC, want_minC)


# ------------------------------------------------------------------------------------------------ the two rule boundaries
@pytest.fixture(params=["0", "2"], ids=["packed", "wide-rows"])
def wide_mode(request, monkeypatch):
    """FSGM_PYD_WIDE: both mappings of the row-packed aggregation kernel for the horizontal lines (tests/test_gpu_pyd.py)."""
    monkeypatch.setenv("FSGM_PYD_WIDE", request.param)
    return request.param


def _peak_along_rows(Cv, mv, Sx, Sy, P1, P2):
    """The largest value the reference forms before it narrows to u8 on the pass-0 paths along x (calc_pyd_cost_sgm.cpp:34-89,
    by tests/py_restatement.py's pyd_step): the previous minimum + P2 (:50-53) and, for every cell that some candidate reads
    as a neighbour, its path cost + P1 (:73)."""
    H, W, D = Cv.shape
    peak = 0
    for y in range(H):
        L = [int(v) for v in Cv[y, 0]] + [0]
        for x in range(1, W):
            dx, dy = mv[0, y, x] - mv[0, y, x - 1], mv[1, y, x] - mv[1, y, x - 1]
            peak = max(peak, L[D] + P2)
            for sx in range(Sx):
                for sy in range(Sy):
                    xpre, ypre = P._trunc(sx + dx + 0.5), P._trunc(sy + dy + 0.5)
                    for k in range(-2, 3):
                        for m in range(-2, 3):
                            tx, ty = xpre + m, ypre + k
                            if (m or k) and 0 <= tx < Sx and 0 <= ty < Sy:
                                peak = max(peak, L[tx * Sy + ty] + P1)
            L = P.pyd_step(L, Cv[y, x], dx, dy, Sx, Sy, P1, P2)
    return peak


def _two_valued(W, H, D, lo, hi, seed):
    """lo or hi, half each; every candidate of the pixels with x mod 4 == 1 is hi (behind R.window_hints' "steps" the minimum
    of their path costs is then hi + P2)."""
    Cv = np.where(synth.uniform_f64(seed, (H, W, D)) < 0.5, lo, hi).astype(np.uint8)
    Cv[:, 1::4, :] = hi
    return np.ascontiguousarray(Cv)


# P1, P2, the volume's maximum: the budget max C + P2 + max(P1, P2) at 255 (row-packed kernels) and at 256 (generic, wrapping)
BUDGETS = [(6, 100, 55), (6, 100, 56), (200, 31, 24), (201, 31, 24)]


@pytest.mark.parametrize("P1,P2,cmax", BUDGETS)
@pytest.mark.parametrize("window", (0, 1))
def test_no_wrap_budget_on_uploaded_volumes(gpu_lib, oracle, wide_mode, window, P1, P2, cmax):
    (rX, rY), (W, H) = R.RULE_WINDOWS[window], (7, 3)
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    total = cmax + P2 + max(P1, P2)
    assert total in (255, 256) and _nowrap(P1, P2, cmax) == (total == 255)
    I1, I2, _ = _frame(W, H, "zero", 11)
    mv = R.window_hints(W + 2, H + 1, "steps", 0)
    Cv = _two_valued(W, H, Sx * Sy, 3, cmax, seed=13 + window)
    assert Cv.max() == cmax
    # the budget is used up: at 255 the largest value before narrowing is 255 itself, at 256 the reference wraps to 0
    peak = _peak_along_rows(Cv, mv, Sx, Sy, P1, P2)
    assert peak == 255 if total == 255 else peak >= 256
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2) as plan:
        plan.set_params(P1, P2, 1, 2, 0, 1)
        _run_uploaded(plan, 0, I1, I2, mv, Cv)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        _compare(plan, 0, oracle, I1, Cv, mv, Sx, Sy, P1, P2, 1, 2, 0)


@pytest.mark.parametrize("P1,P2", [(116, 115), (117, 115)])
@pytest.mark.parametrize("window", (0, 1))
def test_no_wrap_budget_through_the_cost_stage(gpu_lib, oracle, wide_mode, window, P1, P2):
    """A volume built by the cost stage counts as max C = 24 (census 5x5 Hamming mean); here it reaches 24."""
    (rX, rY), (W, H) = R.RULE_WINDOWS[window], (16, 7)
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    total = 24 + P2 + max(P1, P2)
    assert total in (255, 256) and _nowrap(P1, P2, 24) == (total == 255)
    assert pyd.launch_lds(rX, rY, 0)["cost_kernel"] == "rows"
    I1, I2 = R.budget_images(W, H)
    mv = R.window_hints(W + 2, H + 1, "zigzag", 0)
    Cv = oracle.pyd_cost(oracle.census(I1), oracle.census(I2), mv, 0, rX, rY)
    assert Cv.max() == 24
    peak = _peak_along_rows(Cv, mv, Sx, Sy, P1, P2)
    assert peak == 255 if total == 255 else peak >= 256
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 0) as plan:
        plan.set_params(P1, P2, 1, 2, 0, 1)
        plan.upload(0, I1, I2, mv)
        plan.run(STAGE_ALL)
        np.testing.assert_array_equal(plan.download_cost(0), Cv)
        _compare(plan, 0, oracle, I1, Cv, mv, Sx, Sy, P1, P2, 1, 2, 0)


@pytest.mark.parametrize("volume", ("constant255", "two-valued", "high"))
@pytest.mark.parametrize("diag,passes", R.WINDOW_PASSES)
@pytest.mark.parametrize("window", (0, 1))
def test_wta_sums_around_the_u16_bound(gpu_lib, oracle, wide_mode, window, diag, passes, volume):
    """totalPass 64 / 65 with diagonals and 128 / 129 without: the last pass counts at which the weighted sums of u8 path
    costs fit u16 (the row-packed WTA), and the first at which they do not; 257: a weight above a byte; 0: no path slot.
    The row-packed WTA keeps each sum twice: as u32 for the minimum, its index and the tap, and as u16 in LDS for the parabolas'
    neighbours.  On the constant volume every parabola is 0 whatever the neighbours hold, so a sum beyond u16 shows only on
    the "high" volume: costs 250..255 with P1 = P2 = 0, where every path cost is the cost itself, the sums differ from candidate
    to candidate, and past the bound a best candidate with a parabola has a neighbour whose sum exceeds 65535."""
    (rX, rY), (W, H) = R.RULE_WINDOWS[window], R.RULE_FRAMES[window]
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    assert _rows_wta(Sx, Sy, diag, passes) == ((diag, passes) in ((1, 64), (0, 128), (1, 0), (0, 0)))
    I1, I2, mv = _frame(W, H, "general", 17)
    if volume == "constant255":
        P1, P2, Cv = 0, 0, np.full((H, W, Sx * Sy), 255, np.uint8)
    elif volume == "high":
        P1, P2, Cv = 0, 0, (250 + synth.uniform_u8(23, (H, W, Sx * Sy), hi=5)).astype(np.uint8)
        assert Cv.min() == 250 and Cv.max() == 255
    else:
        P1, P2, Cv = 6, 32, _two_valued(W, H, Sx * Sy, 2, 24, seed=19)
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2) as plan:
        plan.set_params(P1, P2, diag, passes, 0, 1)
        _run_uploaded(plan, 0, I1, I2, mv, Cv)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        S = _compare(plan, 0, oracle, I1, Cv, mv, Sx, Sy, P1, P2, diag, passes, 0)
    if volume == "high":
        nd = (4 if diag else 2) * passes
        assert (S == nd * Cv.astype(np.uint32)).all()                      # every path cost is the cost itself
        bd, _, _ = oracle.pyd_wta(S, Sx, Sy, 1)
        dx, dy = bd // Sy, bd % Sy
        Sp = np.pad(S.reshape(H, W, Sx, Sy), ((0, 0), (0, 0), (1, 1), (1, 1)))      # zero ring: a side without a parabola
        yy, xx = np.mgrid[0:H, 0:W]
        beside = np.stack([Sp[yy, xx, dx, dy + 1] * ((dx > 0) & (dx < Sx - 1)), Sp[yy, xx, dx + 2, dy + 1] * ((dx > 0) & (dx < Sx - 1)),
                           Sp[yy, xx, dx + 1, dy] * ((dy > 0) & (dy < Sy - 1)), Sp[yy, xx, dx + 1, dy + 2] * ((dy > 0) & (dy < Sy - 1))])
        # a parabola's neighbour beyond u16 exactly where the sums no longer fit it
        assert (beside > 65535).any() == (nd * 255 > 65535)
    if volume == "constant255":                       # every path cost stays 255: 65280 at the bound, the top of the u16 sums
        assert (S == 255 * (4 if diag else 2) * passes).all()
        if (diag, passes) in ((1, 64), (0, 128)):
            assert S[0, 0, 0] == 65280
