"""The CPU oracle against the reference's own compiled MEX code (oracle/_ref/ref_*.so: the four MEX sources built unmodified by
oracle/Makefile against the stand-in runtime of oracle/refmex/, called through oracle/pyref.py).

Every output array the reference's mexFunction writes is compared with the oracle bit for bit (assert_array_equal: NaNs of the
fp64 planes must sit in the same places); the line it prints is compared with what the gateway tests expect.  No pixel is
excluded anywhere.

The cases come from tests/ref_cases.py: the parametrisations of test_gpu_epi.py / test_gpu_pyd.py / test_gpu_ng.py read from
those tests' own marks, the draws of test_gpu_fuzz.py (tests/fuzz_configs.py, same seeds), edge values (hint maps smaller and
larger than the image, 1xN / Nx1 / 2x2 / 1x1 frames, penalties up to 255, totalPass 1-3, diagonals and adaptive P2 on and off,
halfSearchWinSize 0-2, hints at +-2^31, 3e9, 2^30-1 and around +-0x3FF0), and one KITTI-shaped case per MEX file.

These tests skip where oracle/_ref/ holds no reference binaries (a machine without the reference tree); the fixtures those
binaries wrote are compared unconditionally in tests/test_ref_golden_cpu.py and tests/test_gpu_ref_golden.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyref
from tests import ref_cases as R

_pool = ThreadPoolExecutor(1)


def _need(name):
    if not pyref.available(name):
        pytest.skip(f"oracle/_ref/ref_{name}.so is not built (no reference tree on this machine); "
                    "the reference-written fixtures are checked in tests/test_ref_golden_cpu.py")


def _both(ref_fn, oracle_fn):
    """The reference in a worker thread (one reference call at a time: its runtime keeps one print buffer and libc one rand()
    state), the oracle meanwhile in this one.  Only for wall time: run one after the other, these tests take 60 s instead of 35 s.
    ctypes releases the interpreter lock during either call, the oracle never calls rand(), and the stream handed to the oracle
    is drawn before the reference's srand."""
    fut = _pool.submit(ref_fn)
    want = oracle_fn()
    return fut.result(), want


def _ids(cases):
    return [c[0] for c in cases]


def _same(got, want, names):
    assert len(got) == len(want) == len(names)
    for g, w, n in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, n
        np.testing.assert_array_equal(g, w, err_msg=n)


# ------------------------------------------------------------------------------------------------ calc_cost_sgm
def _check_epi(oracle, build):
    a = build()
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = a
    (ref, printed), want = _both(lambda: pyref.call_calc_cost_sgm(*a), lambda: oracle.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, 4))
    _same(ref[:2], want, ("bestD", "minC"))
    assert not ref[2].any() and not ref[3].any()            # conf, bestD2: created and left zero (calc_cost_sgm.cpp:589-590)
    assert printed == ""


EPI = R.epi_cases() + R.epi_edge_geometry_cases() + R.epi_fuzz_cases() + [R.KITTI_EPI_CPU]


@pytest.mark.parametrize("build", [c[1] for c in EPI], ids=_ids(EPI))
def test_calc_cost_sgm_oracle_equals_reference(oracle, build):
    """calc_cost_sgm: bestD (vz index * 256 with the parabola, then vz -> disparity) and minC.  The reference is 4-path and always
    sub-pixel, so this pins the oracle's paths=4, subpixel=1, vz_to_disp=1 row only: its 8-path aggregation and its subpixel=0 /
    vz_to_disp=0 rows have no reference counterpart and stay unpinned.  Path counts, batch sizes and synthetic
    cost volumes of the GPU parametrisations do not map onto MEX arguments; their shapes, disparity ranges and penalties do.
    207 cases: 146 from test_gpu_epi.py's parametrisations, the edge values and the 4-path penalty sets of
    tests/test_gpu_fused_budgets.py (P1 + P2 = 127, P1 = 0, P1 = P2, ... at D = 16 and 128); 20, every frame of the ten seeds of
    test_gpu_edge_sweeps.py::test_epipolar_random_geometries (tests/edge_inputs.py: epipoles inside, outside, far away and on a
    pixel -- NaN directions, zero offsets --, H = I, both direction flags, 1xN and 63/64/65 shapes, flat and saturated images);
    40 from the two random sweeps' draws (24 + 16 seeds); and the KITTI shape with D = 64 at its full width of 1242 and 64 of
    its 375 rows: the suite has no slow marker, and the full frame costs 5 s here (tests/test_gpu_ref_golden.py runs it at full
    size, D = 128, when the binaries are present)."""
    _need("calc_cost_sgm")
    _check_epi(oracle, build)


# ------------------------------------------------------------------------------------------------ calc_pyd_cost_sgm
PYD = R.pyd_cases() + R.pyd_fuzz_cases() + [R.KITTI_PYD_CPU] + R.pyd_window_cases()


@pytest.mark.parametrize("build", [c[1] for c in PYD], ids=_ids(PYD))
def test_calc_pyd_cost_sgm_oracle_equals_reference(oracle, build):
    """calc_pyd_cost_sgm: bestD, minC, mvSub and the printed line.  362 cases: 56 from test_gpu_pyd.py's parametrisations and
    the edge values (two of them on tests/edge_inputs.py's image pairs: strong gradients, a saturated area), 12 from the random
    sweep's draws, and the KITTI shape (5x5 window) at its full width of 1242 and 32 of its 375 rows: the suite has no slow marker, and the full frame costs 18 s here;
    and 293 at search windows from 13x9 to 63x15 and 31x33 = 1023 candidates on frames of a few pixels, the whole-MEX counterparts of
    tests/test_gpu_pyd_windows.py (tests/ref_cases.py: pyd_window_cases), totalPass 0 / 64 / 65 / 128 / 129 / 257 among them."""
    _need("calc_pyd_cost_sgm")
    a = build()
    I1, I2, mv, rX, rY = a[:5]
    (ref, printed), want = _both(lambda: pyref.call_calc_pyd_cost_sgm(*a), lambda: oracle.calc_pyd_cost_sgm(*a))
    _same(ref, want, ("bestD", "minC", "mvSub"))
    H, W = I1.shape
    assert printed == f"width: {W}, height: {H}, dMax: {(2 * rX + 1) * (2 * rY + 1)}, winRadiusAgg: {a[5]}\n"


# ------------------------------------------------------------------------------------------------ calc_pyd_cost_sgm_ng
NG = R.ng_cases() + R.ng_fuzz_cases() + [R.KITTI_NG_CPU]


@pytest.mark.parametrize("build", [c[1] for c in NG], ids=_ids(NG))
def test_calc_pyd_cost_sgm_ng_oracle_equals_reference(oracle, build):
    """calc_pyd_cost_sgm_ng: minC, the flow and the printed line.  87 cases: 70 from test_gpu_ng.py's parametrisations (batched
    ones contribute each of their frames) and the edge values (two of them on tests/edge_inputs.py's image pairs), 16 from the random sweep's draws, and the KITTI shape.  That one
    keeps the full width and 8 rows (the full frame costs 100 s here; tests/test_gpu_ref_golden.py runs the config-4 level at full
    size against the reference when the binaries are present)."""
    _need("calc_pyd_cost_sgm_ng")
    a = build()
    (ref, printed), want = _both(lambda: pyref.call_calc_pyd_cost_sgm_ng(*a), lambda: oracle.calc_pyd_cost_sgm_ng(*a))
    _same(ref, want, ("minC", "flow"))
    H, W = a[0].shape
    assert printed.startswith(f"width: {W}, height: {H}, dMax: {9 * (2 * a[3] + 1) ** 2}, ")


# The frames of tests/test_gpu_ng_forms.py at 9 and at 441 candidates (halfSearchWinSize 0 and 3): the windows the GPU forms are
# compared with the oracle at, the oracle itself against the reference's compiled code
def _ng_window_case(W, H, i, kind, amp, r, sub, P1, P2, oracle, mv_shape=None):
    from tests.ng_helpers import ng_frame
    a = ng_frame(W, H, i, kind, amp, mv_shape=mv_shape) + (r, 2, sub, P1, P2)
    (ref, printed), want = _both(lambda: pyref.call_calc_pyd_cost_sgm_ng(*a), lambda: oracle.calc_pyd_cost_sgm_ng(*a))
    _same(ref, want, (f"minC {W}x{H} frame {i} {kind} r{r} sub{sub} P{P1},{P2}", "flow"))
    assert printed.startswith(f"width: {W}, height: {H}, dMax: {9 * (2 * r + 1) ** 2}, ")


@pytest.mark.parametrize("W,H", [(61, 37), (29, 28), (28, 57), (27, 5), (1, 12), (12, 1)])
def test_calc_pyd_cost_sgm_ng_oracle_equals_reference_at_9_candidates(oracle, W, H):
    _need("calc_pyd_cost_sgm_ng")
    for kind, amp in (("zero", 1.0), ("int", 2.0), ("general", 0.8)):
        for i in range(8 if (W, H) == (61, 37) else 3):
            for sub, P1, P2 in ((0, 6, 32), (1, 6, 32), (0, 90, 120), (1, 90, 120)):
                _ng_window_case(W, H, i, kind, amp, 0, sub, P1, P2, oracle)
    if (W, H) == (61, 37):
        for mv_shape in ((50, 30), (70, 45)):
            for i in range(3):
                _ng_window_case(W, H, i, "general", 0.8, 0, 1, 6, 32, oracle, mv_shape=mv_shape)


@pytest.mark.parametrize("sub", (0, 1))
@pytest.mark.parametrize("P1,P2", ((6, 32), (90, 120)))
def test_calc_pyd_cost_sgm_ng_oracle_equals_reference_at_441_candidates(oracle, P1, P2, sub):
    _need("calc_pyd_cost_sgm_ng")
    for W, H in ((21, 15), (1, 12), (12, 1)):
        for i in range(3):
            _ng_window_case(W, H, i, "int", 2.0, 3, sub, P1, P2, oracle)


# ------------------------------------------------------------------------------------------------ calc_cost_sgm_ng
OTF = R.otf_cases() + R.otf_fuzz_cases() + [R.KITTI_OTF]


@pytest.mark.parametrize("build", [c[1] for c in OTF], ids=_ids(OTF))
def test_calc_cost_sgm_ng_oracle_equals_reference(oracle, build):
    """calc_cost_sgm_ng after libc srand(seed): minC, the flow and the printed line.  The oracle is handed the values libc rand()
    itself returns after the same srand (pyref.libc_rand_stream), so the pin holds for glibc's stream.  36 cases: 19 from
    test_gpu_ng.py and the edge values (one on tests/edge_inputs.py's image pair), 16 from the random sweep's draws, and 160x120, the largest size the GPU suite runs this
    variant at."""
    _need("calc_cost_sgm_ng")
    I1, I2, P1, P2, seed = build()
    H, W = I1.shape
    rs = pyref.libc_rand_stream(oracle.sgm_ng_rand_draws(W, H), seed)
    (ref, printed), want = _both(lambda: pyref.call_calc_cost_sgm_ng(I1, I2, P1, P2, seed), lambda: oracle.calc_cost_sgm_ng(I1, I2, P1, P2, rs))
    _same(ref, want, ("minC", "flow"))
    assert printed == "dMax : 108\n"
