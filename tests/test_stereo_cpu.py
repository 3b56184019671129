"""CPU tests of the linear build of calc_cost_sgm and of rectified stereo: the numpy restatement (tests/stereo_restatement.py)
against the reference's own code compiled without USE_VZIND (tests/golden/ref_mex_calc_cost_sgm_linear.npz) and against its
closed form on rectified maps; the new structs' mirrors; argument validation of the Python and MEX entry points, all of which
answer before a device is touched (the torch entry points: tests/test_stereo_torch_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from fsgm_amd import _lib, synth
import fsgm_amd
from tests import mexharness as mh
from tests import stereo_restatement as R
from tests.stereo_restatement import golden_case

HERE = os.path.dirname(os.path.abspath(__file__))
N_CASES = R.golden_count()


def test_fixture_holds_the_cases_the_kernels_can_go_wrong_at():
    ids = [golden_case(i)[0]["id"] for i in range(N_CASES)]
    assert 8 <= N_CASES <= 12
    assert any("left" in s for s in ids) and any("right" in s for s in ids) and any("slanted" in s for s in ids)
    assert any(c["I1"].shape[1] < c["D"] for c, _ in map(golden_case, range(N_CASES)))           # W < dMax
    assert any(((o[0] >> 8) == c["D"] - 1).any() for c, o in map(golden_case, range(N_CASES)))   # a winner at dMax - 1
    assert any((c["P1"], c["P2"]) == (100, 200) for c, _ in map(golden_case, range(N_CASES)))    # wrapping penalties
    path = os.path.join(HERE, "golden")
    assert os.path.getsize(os.path.join(path, "ref_mex_calc_cost_sgm_linear.npz")) <= os.path.getsize(os.path.join(path, "ref_mex_calc_cost_sgm.npz"))


@pytest.mark.parametrize("i", range(N_CASES))
def test_restatement_matches_the_reference_built_without_vzind(i):
    c, (bestD, minC, conf, bestD2) = golden_case(i)
    rb, rm = R.calc_cost_sgm_linear(c["I1"], c["I2"], c["D"], c["pd0"], c["nd"], c["P1"], c["P2"], paths=4, subpixel=1)
    assert np.array_equal(rm, minC), c["id"]
    assert np.array_equal(rb, bestD), c["id"]
    assert not conf.any() and not bestD2.any()               # the reference's check is commented out (:589-590)


@pytest.mark.parametrize("W,H,D", [(1, 1, 16), (5, 7, 16), (61, 9, 32), (37, 5, 24)])
@pytest.mark.parametrize("direction", [-1, 1])
def test_restatement_on_rectified_maps_is_the_closed_form(W, H, D, direction):
    I1, I2 = synth.image_pair(W, H, D, seed=W + H)
    pd0, nd = R.rectified_maps(W, H, direction)
    assert np.array_equal(R.linear_raw_cost(I1, I2, D, pd0, nd), R.rectified_raw_cost(I1, I2, D, direction))
    p2, n2 = fsgm_amd.stereo_maps(W, H, direction)
    assert np.array_equal(p2, pd0) and np.array_equal(n2, nd)


def test_box_mean_is_the_reference_expression():
    raw = synth.uniform_u8(3, (6, 7, 4), hi=24)
    H, W, D = raw.shape
    want = np.zeros_like(raw)
    for y in range(H):
        for x in range(W):
            s = np.zeros(D, np.uint32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    s += raw[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
            want[y, x] = (1.0 * s / 25 + 0.5).astype(np.uint8)                                  # :404
    assert np.array_equal(R.box_mean(raw), want)


def test_fb_restatement_on_a_constant_disparity():
    """d = 3 everywhere, direction -1: the four cells around x - 3 are hit by x and x + 1; every pixel whose target lies inside
    is consistent, the first three columns fall outside."""
    W, H = 12, 4
    pd0, nd = R.rectified_maps(W, H, -1)
    D1 = np.full((H, W), 3 << 8, np.uint32)
    conf, D2 = R.linear_fb_check(D1, pd0, nd)
    assert (conf[:, 3:] == 1).all() and (conf[:, :3] == 0).all()
    assert (D2[:, : W - 2] == 3 << 8).all() and (D2[:, W - 2:] == R.INVALID_DISPARITY).all()


def test_stereo_params_default_and_mirrors():
    lib = _lib.load()
    p = lib.fsgm_stereo_params_default()
    assert (p.paths, p.subpixel, p.fb_check, p.direction, p.device) == (4, 1, 0, -1, 0)
    assert [f[0] for f in _lib.StereoParams._fields_] == ["paths", "subpixel", "fb_check", "direction", "device"]
    assert C.sizeof(_lib.StereoParams) == 20 and C.sizeof(_lib.EpiParams) == 20                  # EpiParams unchanged
    e = lib.fsgm_epi_params_default()
    assert (e.paths, e.subpixel, e.vz_to_disp, e.device, e.fb_check) == (4, 1, 1, 0, 0)
    assert (_lib.SAMPLING_VZ, _lib.SAMPLING_LINEAR, _lib.SAMPLING_RECTIFIED) == (0, 1, 2)


def test_c_entry_points_validate_before_touching_a_device():
    lib = _lib.load()
    I = np.zeros((4, 5), np.uint8)
    o = np.zeros((4, 5), np.uint32)
    call = lambda *a: lib.fsgm_stereo_sgm_host(*a)               # noqa: E731
    assert call(0, _lib.ptr(I), _lib.ptr(I), 5, 4, 16, 6, 64, None, _lib.ptr(o), _lib.ptr(o), None, None) == 1
    assert call(1, None, _lib.ptr(I), 5, 4, 16, 6, 64, None, _lib.ptr(o), _lib.ptr(o), None, None) == 1
    assert call(1, _lib.ptr(I), _lib.ptr(I), 5, 4, 0, 6, 64, None, _lib.ptr(o), _lib.ptr(o), None, None) == 1
    prm = lib.fsgm_stereo_params_default()
    prm.direction = 0
    assert call(1, _lib.ptr(I), _lib.ptr(I), 5, 4, 16, 6, 64, C.byref(prm), _lib.ptr(o), _lib.ptr(o), None, None) == 1
    assert b"direction" in lib.fsgm_last_error()
    h = C.c_void_p()
    assert lib.fsgm_epi_plan_create_sampling(C.byref(h), 5, 4, 16, 1, None, 3, -1) == 1
    assert lib.fsgm_epi_plan_create_sampling(C.byref(h), 5, 4, 16, 1, None, _lib.SAMPLING_RECTIFIED, 0) == 1
    assert lib.fsgm_calc_cost_sgm_linear_host(None, None, None) == 1


def test_python_entry_points_validate_their_arguments():
    I1, I2 = synth.image_pair(12, 8, 16)
    with pytest.raises(TypeError):
        fsgm_amd.stereo_sgm(I1.astype(np.float32), I2, 16)
    with pytest.raises(TypeError):
        fsgm_amd.stereo_sgm(I1, I2[:, :-1], 16)
    with pytest.raises(TypeError):
        fsgm_amd.stereo_sgm(I1[0], I2[0], 16)
    with pytest.raises(ValueError, match="direction"):
        fsgm_amd.stereo_sgm(I1, I2, 16, direction=0)
    with pytest.raises(ValueError, match="paths"):
        fsgm_amd.stereo_sgm(I1, I2, 16, paths=5)
    with pytest.raises(ValueError, match="dMax"):
        fsgm_amd.stereo_sgm(I1, I2, 0)
    pd0, nd = fsgm_amd.stereo_maps(12, 8)
    with pytest.raises(TypeError):
        fsgm_amd.calc_cost_sgm_linear(I1, I2, 16, pd0[0], nd, 6, 64)
    with pytest.raises(TypeError):
        fsgm_amd.calc_cost_sgm_linear(I1, I2, 16, pd0.astype(np.float32), nd, 6, 64)
    with pytest.raises(TypeError):
        fsgm_amd.calc_cost_sgm_linear(I1.astype(np.int32), I2, 16, pd0, nd, 6, 64)


def _gateway_args(W=16, H=10, D=16):
    I1, I2 = synth.image_pair(W, H, D)
    pd0, nd, off = synth.epi_maps(W, H)
    return [I1, I2, D, 0.3, pd0, nd, off, 6, 64]


def test_linear_gateway_exports_mexfunction_and_validates():
    mh.stub()
    lib = C.CDLL(os.path.join(mh.MEXDIR, "calc_cost_sgm_linear.mexstub.so"))
    assert hasattr(lib, "mexFunction")
    a = _gateway_args()
    for nlhs, args, ident in ((2, a[:8], "fsgm:nrhs"), (2, a + [1], "fsgm:nrhs"), (5, a, "fsgm:nlhs")):
        with pytest.raises(mh.MexError) as e:
            mh.call("calc_cost_sgm_linear", nlhs, *args)
        assert e.value.ident == ident
    for k, v, ident in ((0, a[0].astype(np.float64), "fsgm:class"), (1, a[1][:, :-1], "fsgm:size"), (4, a[4][0], "fsgm:size"),
                        (5, a[5].astype(np.float32).astype(np.uint8), "fsgm:class"), (6, a[6][:-1], "fsgm:size"), (2, 0, "fsgm:range")):
        b = list(a)
        b[k] = v
        with pytest.raises(mh.MexError) as e:
            mh.call("calc_cost_sgm_linear", 2, *b)
        assert e.value.ident == ident, (k, e.value)


def test_linear_gateway_without_a_gpu_is_a_mex_error():
    if _lib.load().fsgm_device_count() > 0:
        pytest.skip("a GPU is visible")
    for nlhs in (0, 1, 4):
        with pytest.raises(mh.MexError) as e:
            mh.call("calc_cost_sgm_linear", nlhs, *_gateway_args())
        assert e.value.ident == "fsgm:hip" and "no HIP device" in str(e.value)
