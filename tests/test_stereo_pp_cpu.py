"""CPU tests of the rectified-stereo post-processing chain: the restatement pinned to the oracle, the refusals that are answered
before a device is touched, the LDS report, and the conditions under which the GPU tests' inputs mean something.

Shares found on the restatement for the whole calls of tests/stereo_pp_restatement.py:CALLS (lost to the check / kept after
island removal / pixels the in-fill fills, per frame):
  96x40 n1 p4 s1 a0 dmin 0  dir-1        11.1 % / 88.6 % / 438
  96x40 n3 p8 s1 a1 dmin-5  dir-1        4.6, 8.0, 6.5 % / 92.9, 91.5, 92.0 % / 273, 325, 306
  96x40 n1 p8 s0 a0 dmin12  dir+1        12.5 % / 87.5 % / 480
  96x40 n3 p4 s1 a0 dmin12  dir-1 chain  23.6, 25.3, 23.9 % / 76.1, 74.7, 75.7 % / 918, 972, 932
  61x37 n3 p4 s0 a1 dmin-5  dir+1        8.2 % / 91.8 % / 185 each
  61x37 n1 p8 s1 a0 dmin 0  dir-1 chain  10.9 % / 89.1 % / 247
  61x37 n1 p4 s1 a0 dmin12  dir+1        30.9 % / 69.1 % / 697
(subpixel = 0 leaves the matcher's bestD the reference's unscaled index, so those frames lose their border columns only.)
Two-plane map 64x5: the check removes 72 (direction -1) / 75 (+1) of 320 pixels."""
import ctypes as C

import numpy as np
import pytest

from fsgm_amd import _lib, stereo_pp, synth
from oracle import pyoracle
from tests import stereo_pp_restatement as P

FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    m = ~np.isnan(want)
    assert np.array_equal(got[m].view(np.uint64), want[m].view(np.uint64)), f"{what}: values differ"


@pytest.mark.parametrize("kind,seed", [("general", 7), ("general", 8), ("radial", 9), ("axis", 10)])
def test_restatement_is_the_oracle_with_the_vz_disparity_function(kind, seed):
    W, H, vMax, n = 40, 30, 0.3, 65.0
    pd0, nd, off = synth.epi_maps(W, H, kind, seed=seed)
    u = synth.uniform_f64(seed + 100, (2, H, W))
    D1 = np.floor(u[0] * 64 * 256) / 256.0                      # vz indices in 1/256 steps, targets inside and outside the image
    D1[u[1] < 0.12] = np.nan
    D1[3, 4:9] = 0.0
    vz = P.vz_disp(off, vMax, n)
    D2 = P.disp_from_first(D1, pd0, nd, vz)
    want2 = pyoracle.calc_disp_from_first(D1, pd0, nd, off, vMax, n)
    _same(D2, want2, "calc_disp_from_first")
    assert (want2 == -1).any() and (want2 >= 0).any()
    out = P.fb_check(D1, D2, pd0, nd, vz)
    want = pyoracle.forward_backward_check(D1, want2, pd0, nd, off, vMax, n)
    _same(out, want, "forward_backward_check")
    lost = ~np.isnan(D1) & np.isnan(want)
    assert lost.any() and (~np.isnan(want)).any()
    # a second-view map that is not the first map's own: every branch of the check
    other = np.roll(want2, 3, axis=1)
    _same(P.fb_check(D1, other, pd0, nd, vz), pyoracle.forward_backward_check(D1, other, pd0, nd, off, vMax, n), "check, foreign D2")


def test_stereo_form_is_the_generic_one_on_rectified_maps():
    # the closed statement of one row, for the reader: a constant map of index k lands k + d_min columns along the direction
    w = np.full((3, 20), 2.0)
    D2 = P.stereo_disp_from_first(w, 3, -1)
    assert (D2[:, :16] == 2.0).all() and (D2[:, 16:] == -1.0).all()            # 1-based targets x + 1 - 5 and the column after it
    c = P.stereo_fb_check(w, D2, 3, -1)
    assert np.isnan(c[:, :5]).all() and (c[:, 5:] == 2.0).all()                # x + 1 - 5 < 1 leaves the image
    D2 = P.stereo_disp_from_first(w, -7, +1)                                   # disp -5, direction +1: the same targets
    assert (D2[:, :16] == 2.0).all() and (D2[:, 16:] == -1.0).all()


def _pp_call(lib, W=5, H=4, D=16, d_min=0, prm=None, pp=None, n=1):
    I = np.zeros((n, H, W), np.uint8) if W * H * n < 1 << 20 else np.zeros(1, np.uint8)
    out = np.full((n, H, W), 7.0) if W * H * n < 1 << 20 else np.zeros(1)
    st = lib.fsgm_stereo_sgm_pp_host(n, _lib.ptr(I), _lib.ptr(I), W, H, D, 6, 64, prm, None, d_min, pp, _lib.ptr(out), None, None, None, None)
    return st, out


def test_refusals_without_a_device():
    lib = stereo_pp._lib_bound()
    st, out = _pp_call(lib, W=8193, H=1)
    assert st == FSGM_ERR_UNSUPPORTED and b"8192" in lib.fsgm_last_error() and (out == 7.0).all()
    prm = lib.fsgm_stereo_params_default()
    prm.fb_check = 1
    st, out = _pp_call(lib, prm=C.byref(prm))
    assert st == FSGM_ERR_INVALID and b"fb_check" in lib.fsgm_last_error() and (out == 7.0).all()
    for k in range(7):
        pp = lib.fsgm_stereo_pp_params_default()
        pp.reserved[k] = 1
        st, out = _pp_call(lib, pp=C.byref(pp))
        assert st == FSGM_ERR_INVALID and b"reserved" in lib.fsgm_last_error() and (out == 7.0).all()
    for d_min in (1025, -1025, 1 << 30):
        st, out = _pp_call(lib, d_min=d_min)
        assert st == FSGM_ERR_INVALID and b"d_min" in lib.fsgm_last_error() and (out == 7.0).all()
    # the device form and the stages answer the same way, before any pointer is looked at
    a = np.zeros((1, 8193), np.float64)
    p = _lib.ptr(a)
    assert lib.fsgm_stereo_sgm_pp_device(1, p, p, 8193, 1, 16, 6, 64, None, None, 0, None, p, None, None, None, None, None, None) == FSGM_ERR_UNSUPPORTED
    assert lib.fsgm_stereo_disp_from_first_host(1, p, 8193, 1, 0, -1, p, 0) == FSGM_ERR_UNSUPPORTED
    assert lib.fsgm_stereo_disp_from_first_device(1, p, 8193, 1, 0, -1, p, 0, None, None) == FSGM_ERR_UNSUPPORTED
    assert lib.fsgm_stereo_fb_check_host(1, p, None, 8193, 1, 0, -1, 2.0, p, None, 0) == FSGM_ERR_UNSUPPORTED
    assert lib.fsgm_stereo_fb_check_device(1, p, None, 8193, 1, 0, -1, 2.0, p, None, 0, None, None) == FSGM_ERR_UNSUPPORTED
    assert lib.fsgm_stereo_fb_check_host(1, p, None, 5, 1, 1025, -1, 2.0, p, None, 0) == FSGM_ERR_INVALID
    assert lib.fsgm_stereo_fb_check_host(1, p, None, 5, 1, 0, 0, 2.0, p, None, 0) == FSGM_ERR_INVALID and b"direction" in lib.fsgm_last_error()
    assert lib.fsgm_stereo_fb_check_host(1, p, None, 5, 1, 0, -1, -1.0, p, None, 0) == FSGM_ERR_INVALID and b"thr" in lib.fsgm_last_error()
    a[0, 3] = -0.5                                               # a negative value: the host forms answer on the host
    assert lib.fsgm_stereo_disp_from_first_host(1, p, 5, 1, 0, -1, p, 0) == FSGM_ERR_INVALID and b"non-negative" in lib.fsgm_last_error()


def test_defaults_and_python_checks():
    lib = stereo_pp._lib_bound()
    d = lib.fsgm_stereo_pp_params_default()
    assert (d.speckle_max_diff, d.speckle_max_size, d.fb_threshold, d.island_fraction, d.in_fill) == (2.0, 100.0, 2.0, 0.1, 1)
    assert list(d.reserved) == [0] * 7
    I = np.zeros((4, 5), np.uint8)
    with pytest.raises(ValueError, match="d_min"):
        stereo_pp.stereo_sgm_pp(I, I, 16, d_min=2000)
    with pytest.raises(TypeError, match="unknown"):
        stereo_pp.stereo_sgm_pp(I, I, 16, fb_thr=1.0)
    with pytest.raises(ValueError, match="direction"):
        stereo_pp.stereo_sgm_pp(I, I, 16, direction=0)
    with pytest.raises(TypeError, match="float64"):
        stereo_pp.stereo_fb_check(I)


def test_lds_report():
    assert stereo_pp.launch_lds(1) == 8
    assert stereo_pp.launch_lds(8192) == 65536
    with pytest.raises(_lib.FsgmError) as e:
        stereo_pp.launch_lds(8193)
    assert e.value.status == FSGM_ERR_UNSUPPORTED
    with pytest.raises(_lib.FsgmError):
        stereo_pp.launch_lds(0)


@pytest.mark.parametrize("call", P.CALLS, ids=P.call_id)
def test_whole_call_frames_are_not_vacuous(call):
    _, _, _, outs = P.call_reference(call)
    for f, o in enumerate(outs):
        lost, kept, filled = P.shares(o["ch"])
        assert lost >= 0.01, f"frame {f}: the check removes {lost:.3%}"
        assert kept >= 0.25, f"frame {f}: {kept:.3%} kept after island removal"
        assert filled >= 1, f"frame {f}: the in-fill fills nothing"


@pytest.mark.parametrize("direction", [-1, +1])
def test_two_plane_map_has_an_occlusion_band(direction):
    w = P.two_plane_map(64, 5)
    c = P.stereo_fb_check(w, P.stereo_disp_from_first(w, 0, direction), 0, direction)
    removed = int(np.isnan(c).sum())
    assert removed >= 1 and removed <= w.size // 2
    # the band: background pixels whose target lies under the rectangle's second-view footprint
    assert np.isnan(c[w == 4.0]).any()
