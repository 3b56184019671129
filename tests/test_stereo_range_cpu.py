"""CPU tests of rectified stereo with a search range that starts at d_min: the oracle on the shifted maps against the reference's
own compiled linear build (tests/golden/ref_mex_stereo_range.npz), the plain integer statement clamp(x + direction * (d_min + d))
against the oracle, the conditions the shifted pairs of the GPU tests are adopted on, and what answers before a device is touched:
the new entry points' validation, the declared signatures, the Python wrappers' new parameter (the torch wrapper:
tests/test_stereo_range_torch_cpu.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import _lib, synth
from tests import stereo_range_restatement as SR
from tests import stereo_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
N_CASES = SR.golden_count()
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4


def test_fixture_holds_the_cases_the_issue_names():
    cs = [SR.golden_case(i)[0] for i in range(N_CASES)]
    assert len({c["I1"].shape for c in cs}) >= 2
    assert {c["direction"] for c in cs} == {-1, 1}
    assert {c["d_min"] for c in cs} >= {-70, -1, 1, 7, 40}
    assert {c["D"] for c in cs} == {16, 48, 64}
    assert {c["paths"] for c in cs} == {4, 8} and {c["fb"] for c in cs} == {0, 1}
    path = os.path.join(HERE, "golden")
    others = [os.path.getsize(os.path.join(path, p)) for p in os.listdir(path) if p.startswith("ref_mex_") and "stereo_range" not in p]
    assert os.path.getsize(SR.GOLDEN_PATH) <= max(others)


@pytest.mark.parametrize("i", range(N_CASES))
def test_oracle_on_shifted_maps_is_the_reference_on_them(i):
    c, (bestD, minC, conf, bestD2) = SR.golden_case(i)
    o = SR.oracle(c["I1"], c["I2"], c["D"], c["direction"], c["d_min"], c["P1"], c["P2"], paths=c["paths"], fb_check=c["fb"])
    assert np.array_equal(o["minC"], minC), c["id"]
    assert np.array_equal(o["bestD"], bestD), c["id"]
    if c["fb"]:
        assert np.array_equal(o["bestD2"], bestD2), c["id"]
        assert np.array_equal(o["conf"], conf), c["id"]
    else:
        assert not conf.any() and not bestD2.any()               # the reference's check is commented out (:589-590)


@pytest.mark.parametrize("i", range(N_CASES))
def test_closed_form_is_the_oracle_on_the_fixture_cases(i):
    c, (bestD, minC, _, _) = SR.golden_case(i)
    f = SR.closed_form(c["I1"], c["I2"], c["D"], c["direction"], c["d_min"], c["P1"], c["P2"], paths=c["paths"])
    assert np.array_equal(f["minC"], minC) and np.array_equal(f["bestD"], bestD), c["id"]


# the whole window one clamped column on either side (-D - 3, W + 5), the off-by-one pair, a shift across the image
@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("W,H,D,d_min", [(23, 6, 16, -19), (23, 6, 16, 28), (23, 6, 16, -1), (23, 6, 16, 1), (37, 5, 24, 7), (9, 4, 16, -1024),
                                         (9, 4, 16, 1024), (1, 3, 16, 5)])
def test_closed_form_is_the_oracle_at_the_edges(W, H, D, d_min, direction):
    I1, I2 = synth.image_pair(W, H, D, seed=W + D)
    pd0, nd = SR.shifted_maps(W, H, direction, d_min)
    raw = SR.range_raw_cost(I1, I2, D, direction, d_min)
    assert np.array_equal(R.linear_raw_cost(I1, I2, D, pd0, nd), raw)
    if abs(d_min) > W + D:                                       # every candidate of every pixel samples one edge column
        assert (raw == raw[:, :, :1]).all()
    if d_min == 0:
        assert np.array_equal(raw, R.rectified_raw_cost(I1, I2, D, direction))
    a, b = SR.oracle(I1, I2, D, direction, d_min, paths=8), SR.closed_form(I1, I2, D, direction, d_min, paths=8)
    for k in ("C", "S", "bestD", "minC"):
        assert np.array_equal(a[k], b[k]), k


def test_d_min_zero_is_the_unshifted_restatement():
    I1, I2 = synth.image_pair(31, 7, 16, seed=5)
    for direction in (-1, 1):
        assert np.array_equal(SR.range_raw_cost(I1, I2, 16, direction, 0), R.rectified_raw_cost(I1, I2, 16, direction))
        p, n = SR.shifted_maps(31, 7, direction, 0)
        q, m = R.rectified_maps(31, 7, direction)
        assert np.array_equal(p, q) and np.array_equal(n, m)


def test_true_disparity_encoding():
    v = np.array([0, 255, 3 << 8, R.INVALID_DISPARITY], np.uint32)
    assert SR.true_disp(v, -70).tolist() == [-17920, -17665, -17152, 131072 - 17920]
    assert SR.true_disp2(v, 512).tolist() == [131072, 131327, 131840, SR.INT32_MIN]      # 512 << 8 is a VALID disparity at d_min = 512
    assert SR.true_disp2(v, 0).tolist() == [0, 255, 768, SR.INT32_MIN]


@pytest.mark.parametrize("W,H,D,direction,d_min,s,seed", SR.SHIFT_CASES)
def test_shifted_pairs_make_the_shift_matter(W, H, D, direction, d_min, s, seed):
    """The pairs the GPU tests run on: the true disparity s lies outside [0, dMax) and inside [d_min, d_min + dMax); on at least
    half of the interior pixels the oracle's winner is within one index of s - d_min, and at d_min = 0 the same pair gives
    another disp on at least that share."""
    assert not 0 <= s < D and d_min <= s < d_min + D
    I1, I2 = SR.shifted_pair(W, H, s, direction, seed)
    near, differs = SR.shift_matters(I1, I2, D, direction, d_min, s)
    assert near >= 0.5, near
    assert differs >= 0.5, differs


# ---------------------------------------------------------------------------------------------- fail without the feature
def _range_call(lib, d_min, W=5, H=4, D=16, prm=None):
    I = np.zeros((H, W), np.uint8)
    d, m = np.full((H, W), 7, np.int32), np.full((H, W), 7, np.uint32)
    st = lib.fsgm_stereo_sgm_host_range(1, _lib.ptr(I), _lib.ptr(I), W, H, D, 6, 64, prm, None, d_min, _lib.ptr(d), _lib.ptr(m), None, None)
    return st, d, m


def test_host_range_refuses_a_d_min_beyond_the_limit_without_a_device():
    lib = _lib.load()
    for d_min in (1025, -1025, 1 << 30):
        st, d, m = _range_call(lib, d_min)
        assert st == FSGM_ERR_INVALID
        assert b"d_min" in lib.fsgm_last_error()
        assert (d == 7).all() and (m == 7).all()
    # the other arguments are checked as for fsgm_stereo_sgm_host, also before a device
    prm = lib.fsgm_stereo_params_default()
    prm.direction = 0
    assert _range_call(lib, 3, prm=C.byref(prm))[0] == FSGM_ERR_INVALID and b"direction" in lib.fsgm_last_error()
    assert _range_call(lib, 3, D=0)[0] == FSGM_ERR_INVALID
    opt = _lib.options(0)
    opt.reserved[0] = 1
    I = np.zeros((4, 5), np.uint8)
    o = np.zeros((4, 5), np.int32)
    assert lib.fsgm_stereo_sgm_host_range(1, _lib.ptr(I), _lib.ptr(I), 5, 4, 16, 6, 64, None, C.byref(opt), 3, _lib.ptr(o), _lib.ptr(o),
                                          None, None) == FSGM_ERR_INVALID


def test_plan_set_d_min_exists_with_the_declared_signature():
    lib = _lib.load()
    assert lib.fsgm_epi_plan_set_d_min.argtypes == [C.c_void_p, C.c_int32]
    assert lib.fsgm_epi_plan_set_d_min(None, 3) == FSGM_ERR_INVALID          # a null plan: answered, not dereferenced
    with open(os.path.join(os.path.dirname(HERE), "include", "fsgm.h")) as f:
        hdr = re.sub(r"\s+", " ", f.read())
    assert "fsgm_status fsgm_epi_plan_set_d_min(fsgm_epi_plan* plan, int32_t d_min);" in hdr
    assert "#define FSGM_D_MIN_LIMIT 1024" in hdr
    for name, outs in (("host", "int32_t* disp2);"), ("device", "int32_t* disp2, void* stream, int32_t* status);")):
        m = re.search(rf"fsgm_status fsgm_stereo_sgm_{name}_range\(([^;]*);", hdr)
        assert m and "const fsgm_epi_options* opt, int32_t d_min, int32_t* disp, uint32_t* minC, uint8_t* conf, " + outs in m.group(0)
        assert hasattr(lib, f"fsgm_stereo_sgm_{name}_range")
    assert hasattr(fsgm_amd.EpiPlan, "set_d_min")
    # the structs the older entry points take are what they were
    assert C.sizeof(_lib.StereoParams) == 20 and C.sizeof(_lib.EpiParams) == 20 and C.sizeof(_lib.EpiOptions) == 32


def test_python_wrappers_accept_d_min():
    sig = inspect.signature(fsgm_amd.stereo_sgm)
    assert sig.parameters["d_min"].default is None and sig.parameters["d_min"].kind is inspect.Parameter.KEYWORD_ONLY
    I1, I2 = synth.image_pair(12, 8, 16)
    with pytest.raises(ValueError, match="d_min"):
        fsgm_amd.stereo_sgm(I1, I2, 16, d_min=1025)
    with pytest.raises(ValueError, match="d_min"):
        fsgm_amd.stereo_sgm(I1, I2, 16, d_min=-1025)
    with pytest.raises(TypeError, match="d_min"):
        fsgm_amd.stereo_sgm(I1, I2, 16, d_min=1.5)
    with pytest.raises(ValueError, match="direction"):           # the older checks still come first
        fsgm_amd.stereo_sgm(I1, I2, 16, direction=0, d_min=3)
