"""CPU tests of the filtered-flow yardstick: tests/flow_pp_restatement.py against the existing oracle where the two must
coincide, its forward-backward rule against a hand-built map, and the new entry points' argument checks (which answer
before any device is touched)."""
import numpy as np
import pytest

from tests import flow_pp_inputs
from tests import flow_pp_restatement as R
from fsgm_amd import synth


def _same(a, b):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(np.nan_to_num(a), np.nan_to_num(b))


@pytest.mark.parametrize("W,H,seed", [(61, 47, 11), (160, 120, 12), (1, 9, 13), (9, 1, 14)])
@pytest.mark.parametrize("maxDiff,maxSize", [(2, 100), (0.25, 7), (np.inf, 500.0)])
def test_vector_speckle_with_constant_v_is_the_scalar_filter(oracle, W, H, seed, maxDiff, maxSize):
    u = synth.vz_index_map(W, H, 64, seed=seed)
    flow = np.stack([u, np.full_like(u, 1.5)])
    got, dropped = R.flow_speckle_filter(flow, maxDiff, maxSize)
    want, _ = oracle.speckle_filter(u, maxDiff, maxSize)
    _same(got[0], want)
    np.testing.assert_array_equal(dropped, np.isnan(want) & ~np.isnan(u))
    _same(got[1], np.where(dropped, np.nan, 1.5))               # invalid pixels pass through as they are


@pytest.mark.parametrize("W,H,seed", [(61, 47, 21), (160, 120, 22), (1, 9, 23), (9, 1, 24), (1, 1, 25)])
def test_vector_fill_u_plane_is_the_scalar_fill(oracle, W, H, seed):
    u = synth.vz_index_map(W, H, 64, seed=seed, invalid=0.3)
    v = synth.uniform_f64(seed + 5, (H, W)) * 8 - 4
    got = R.flow_in_fill(np.stack([u, v]))
    _same(got[0], oracle.scanline_in_fill(u))
    keep = ~np.isnan(u)
    np.testing.assert_array_equal(got[1][keep], v[keep])                       # only the holes of u are written


def test_fill_takes_the_minimum_per_channel():
    nan = np.nan
    u = np.array([[nan, 3.0, nan, nan, 1.0, nan]])
    v = np.array([[7.0, -2.0, 9.0, nan, 5.0, nan]])
    got = R.flow_in_fill(np.stack([u, v]))
    np.testing.assert_array_equal(got[0], [[3.0, 3.0, 1.0, 1.0, 1.0, 1.0]])
    np.testing.assert_array_equal(got[1], [[-2.0, -2.0, -2.0, -2.0, 5.0, 5.0]])


def test_matlab_round_is_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4, -2.6])
    np.testing.assert_array_equal(R.matlab_round(x), [1, 2, 3, -1, -2, -3, 0, -0.0, 2, -3])


def test_fb_check_of_a_horizontal_flow_against_a_hand_built_map():
    """One row of 8 pixels (MATLAB columns 1..8), v = 0.  b = 0 everywhere except an invalid pixel at column 6."""
    nan = np.nan
    #                i:  1     2     3     4      5     6     7     8
    fu = np.array([[-0.5,  0.5,  1.5, -1.5,   2.0,  0.0,  1.5, -8.5]])
    # i + f:            0.5   2.5   4.5   2.5    7.0   6.0   8.5  -0.5
    # round:            1     3     5     3      7     6     9    -1  (half away from zero: 0.5 -> 1, 8.5 -> 9, -0.5 -> -1)
    f = np.stack([fu, np.zeros_like(fu)])
    b = np.zeros((2, 1, 8))
    b[0, 0, 2] = 1.0          # column 3: partners of pixels 2 (sum 1.5, kept) and 4 (sum -0.5, kept)
    b[0, 0, 4] = 0.5          # column 5: partner of pixel 3, sum 2.0 = thr, kept (the test is >)
    b[0, 0, 6] = 0.25         # column 7: partner of pixel 5, sum 2.25 > thr
    b[:, 0, 5] = nan          # column 6: partner of pixel 6 is invalid
    got, why = R.flow_fb_check(f, b, 2.0)
    want_u = np.array([[-0.5, 0.5, 1.5, -1.5, nan, nan, nan, nan]])
    _same(got[0], want_u)
    _same(got[1], np.where(np.isnan(want_u), nan, 0.0))
    np.testing.assert_array_equal(why["mismatch"], [[0, 0, 0, 0, 1, 0, 0, 0]])
    np.testing.assert_array_equal(why["partner"], [[0, 0, 0, 0, 0, 1, 0, 0]])
    np.testing.assert_array_equal(why["outside"], [[0, 0, 0, 0, 0, 0, 1, 1]])
    # half to even would send pixel 1 to column 0 (outside) and keep pixel 7 at column 8
    assert not why["outside"][0, 0] and why["outside"][0, 6]
    # the mismatch rule is per component: a v sum over thr rejects although u agrees
    f2, b2 = np.zeros((2, 1, 3)), np.zeros((2, 1, 3))
    b2[1, 0, 1] = -2.5
    got2, why2 = R.flow_fb_check(f2, b2, 2.0)
    np.testing.assert_array_equal(why2["mismatch"], [[0, 1, 0]])


@pytest.mark.parametrize("W,H", [(61, 47), (320, 240)])
@pytest.mark.parametrize("kind", ["general", "int", "even", "zero"])
def test_synthetic_pairs_are_rejected_for_every_reason(W, H, kind):
    f, b = flow_pp_inputs.flow_pair(W, H, kind, seed=5)
    pp, c, why = R.chain(f, b)
    for reason in ("outside", "partner", "mismatch", "speckle"):
        assert why[reason].any(), reason
    assert R.valid(c).mean() >= 0.25
    np.testing.assert_array_equal(pp[2], R.valid(c))


def test_entry_points_refuse_bad_arguments():
    import ctypes as C
    from fsgm_amd import _lib, pyramid, post
    lib = _lib.load()
    post._bind(lib)
    pyramid._bind(lib), pyramid._bind_ng(lib), pyramid._bind_flow_pp(lib)
    a = np.zeros((2, 4, 5))
    I = np.zeros((4, 5), np.uint8)
    p = _lib.ptr

    def refused(st, text):
        assert st == 1, (st, lib.fsgm_last_error())
        assert text in lib.fsgm_last_error().decode()

    refused(lib.fsgm_flow_fb_check_host(1, p(a), p(a), 5, 4, -1.0, p(a), 0), "thr")
    refused(lib.fsgm_flow_fb_check_host(1, p(a), None, 5, 4, 2.0, p(a), 0), "null")
    refused(lib.fsgm_flow_speckle_filter_host(0, p(a), 5, 4, 2.0, 100.0, p(a), 0), "n_frames")
    refused(lib.fsgm_flow_in_fill_host(1, p(a), 0, 4, p(a), 0), "width")
    pp = np.zeros((3, 4, 5))
    for field, value, text in (("fb_thr", -0.5, "fb_thr"), ("island_fraction", 1.5, "island_fraction"),
                               ("island_fraction", -0.1, "island_fraction"), ("median", 2, "median"), ("matcher", 7, "matcher")):
        prm = lib.fsgm_flow_pp_params_default(0)
        setattr(prm, field, value)
        refused(lib.fsgm_pyramidal_flow_pp_host(1, p(I), p(I), 5, 4, 1, C.byref(prm), p(pp), None, None, None, None), text)
    prm = lib.fsgm_flow_pp_params_default(1)
    assert (prm.matcher, prm.ng.numPyd, prm.pyd.numPyd) == (1, 3, 5)
    assert (prm.speckle_max_diff, prm.speckle_max_size, prm.fb_thr, prm.island_fraction, prm.median) == (2.0, 100.0, 2.0, 0.1, 0)
    with pytest.raises(ValueError, match="matcher"):
        pyramid.pyramidal_flow_pp(I, I, 3, matcher="census")
    with pytest.raises(TypeError, match="unknown"):
        pyramid.pyramidal_flow_pp(I, I, 3, matcher="ng", aggHalfWinSize=2)
    with pytest.raises(ValueError, match="shape"):
        post.flow_fb_check(a, np.zeros((2, 4, 6)))
