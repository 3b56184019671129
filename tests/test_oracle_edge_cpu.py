"""The CPU oracle (oracle/fsgm_oracle_post.cpp, fsgm_oracle_geometry.cpp) against the second restatements
(tests/py_restatement.py) on the edge-value inputs of the GPU sweeps (tests/edge_inputs.py), at small sizes: ties on maxDiff,
regions one pixel either side of maxSpeckleSize, +-0.0, +Inf, subnormals, huge values, NaN rows / columns / frames, targets on
the border and on round-half points, epipoles on a pixel.  No GPU needed."""
import os

import numpy as np
import pytest

from tests import edge_inputs as E
from tests import py_restatement as R

_SOAK = int(os.environ.get("FSGM_FUZZ_SEEDS", "0"))


def _seeds(default):
    return range(_SOAK if _SOAK > 0 else default)


def _same(a, b, msg=""):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    np.testing.assert_array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0), err_msg=msg)


@pytest.mark.parametrize("seed", _seeds(12))
def test_post_scripts_oracle_vs_restatement(oracle, seed):
    r = E.rng(7000 + seed)
    W, H, N = E.post_shape(r, small=True)
    maxDiff, maxSize, vMax, n, dMax = E.post_params(r)
    D1 = E.post_maps(r, W, H, N, maxSize, vMax, n)
    Pd0, nd, O = E.post_geometry(r, W, H, N)
    for f in range(N):
        msg = f"seed {seed} W{W} H{H} frame {f}/{N} maxDiff {maxDiff} maxSize {maxSize} vMax {vMax} n {n} dMax {dMax}"
        out, labels = oracle.speckle_filter(D1[f], maxDiff, maxSize)
        rout, rlabels = R.speckle_filter(D1[f], maxDiff, maxSize)
        _same(out, rout, msg + " speckle_filter")
        np.testing.assert_array_equal(labels, rlabels, err_msg=msg + " labels")
        with np.errstate(all="ignore"):
            D2 = oracle.calc_disp_from_first(D1[f], Pd0[f], nd[f], O[f], vMax, n)
            _same(D2, R.calc_disp_from_first(D1[f], Pd0[f], nd[f], O[f], vMax, n), msg + " calc_disp_from_first")
            _same(oracle.forward_backward_check(D1[f], D2, Pd0[f], nd[f], O[f], vMax, n),
                  R.forward_backward_check(D1[f], D2, Pd0[f], nd[f], O[f], vMax, n), msg + " forward_backward_check")
            _same(oracle.vzind2disp(D1[f], O[f], vMax, n), R.vzInd2Disp(D1[f], O[f], vMax, n), msg + " vzInd2Disp")
        _same(oracle.scanline_in_fill(D1[f]), R.scanline_in_fill(D1[f]), msg + " scanline_in_fill")


def test_fb_check_round_half_and_large_odd_targets(oracle):
    """MATLAB's round is half away from zero and exact: pred(0.5) -> 0, 2.5 -> 3, an odd integer >= 2^52 -> itself.  Targets on those
    values (nd = 0: the target is Pd0 itself) decide whether a pixel is inside the image (forward_backward_check.m:17-22)."""
    W, H = 4, 3
    D1 = np.full((H, W), 1.0)
    D2 = np.full((H, W), 1.0)
    nd, O = np.zeros((2, H, W)), np.zeros((H, W))
    Pd0 = np.ones((2, H, W))
    Pd0[0, 0, :] = [E.pred(0.5), 0.5, E.pred(1.5), W + 0.5]               # 0 (out), 1 (in), 1 (in), W + 1 (out)
    Pd0[0, 1, :] = [2.0 ** 52 + 1, 2.5, -0.5, E.pred(W + 0.5)]            # out, 3 (in), -1 (out), W (in)
    want = np.array([[np.nan, 1, 1, np.nan], [np.nan, 1, np.nan, 1], [1, 1, 1, 1]])
    _same(oracle.forward_backward_check(D1, D2, Pd0, nd, O, 0.3, 65), want)
    _same(R.forward_backward_check(D1, D2, Pd0, nd, O, 0.3, 65), want)
    for v, want in ((E.pred(0.5), 0.0), (0.5, 1.0), (-0.5, -1.0), (E.pred(2.5), 2.0), (2.5, 3.0), (-2.5, -3.0),
                    (2.0 ** 52 + 1, 2.0 ** 52 + 1), (2.0 ** 53 - 1, 2.0 ** 53 - 1), (-(2.0 ** 52 + 1), -(2.0 ** 52 + 1)), (np.inf, np.inf)):
        assert R.matlab_round(v) == want, v                                # the restatement's round (its :17-20)


def test_calc_disp_from_first_keeps_minus_zero(oracle):
    """calc_disp_from_first.m:24-46 with only -0.0 offers: the cell takes -0.0 (-1 < -0.0), so forward_backward_check keeps the
    pixel (:27 d2 == -1 is false).  The oracle and the restatement both follow the MATLAB rule."""
    D1 = np.array([[-0.0, -0.0, 3.0]])
    Pd0 = np.stack([np.array([[1.0, 2.0, 3.0]]), np.ones((1, 3))])
    nd, O = np.zeros((2, 1, 3)), np.ones((1, 3))
    for D2 in (oracle.calc_disp_from_first(D1, Pd0, nd, O, 0.3, 65), R.calc_disp_from_first(D1, Pd0, nd, O, 0.3, 65)):
        assert (D2 == np.array([[0.0, 0.0, 3.0]])).all()
        chk = oracle.forward_backward_check(D1, D2, Pd0, nd, O, 0.3, 65)
        assert not np.isnan(chk).any()


@pytest.mark.parametrize("seed", _seeds(10))
def test_epipolar_maps_oracle_vs_restatement(oracle, seed):
    r = E.rng(7500 + seed)
    W, H = E.epi_shape(r, hi=40)
    F, Hm, epi, direction, where = E.epi_geometry(r, W, H, oracle)
    msg = f"seed {seed} W{W} H{H} epipole {where} {epi} direction {direction}"
    with np.errstate(all="ignore"):
        want = R.epipolar_maps(F, Hm, epi, direction, W, H)
    got = oracle.epipolar_maps(F, Hm, epi, direction, W, H)
    for g, w, name in zip(got, want, ("Pd0", "normlizeDirection", "Offset", "Rflow")):
        _same(g, w, f"{msg} {name}")
    if where == "on_pixel":
        assert (got[2] == 0).any() and np.isnan(got[1]).any(), msg


@pytest.mark.parametrize("seed", _seeds(6))
def test_vmf_oracle_vs_sorted_windows(oracle, seed):
    """vmf.m (medfilt2 5x5, zero padding) with NaN ordered above every number, like MATLAB's sort (the rule this project picked;
    medfilt2's own is unpinned): the 13th entry of np.sort of the padded window, which puts NaN last."""
    r = E.rng(7700 + seed)
    W, H = E.pick_size(r, 1, 30, (1, 2, 3, 4, 5, 6)), E.pick_size(r, 1, 30, (1, 2, 3, 4, 5, 6))
    ch = int(r.randint(1, 4))
    flow = E.vmf_flows(r, W, H, 1, ch)[0]
    pad = np.pad(flow, ((0, 0), (2, 2), (2, 2)))
    win = np.lib.stride_tricks.sliding_window_view(pad, (5, 5), axis=(1, 2)).reshape(ch, H, W, 25)
    want = np.sort(win, axis=-1)[..., 12]
    _same(oracle.vmf(flow), want, f"seed {seed} W{W} H{H} ch{ch}")
