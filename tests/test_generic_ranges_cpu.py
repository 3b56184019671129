"""The disparity ranges that stay on the generic line kernel and the generic WTA (agg_generic_kernel, wta_generic_kernel: every
dMax that is neither 16 << k nor a packed split, up to FSGM_GENERIC_MAX_D = 1024), as far as no device is needed: the CPU oracle
against the reference's own compiled code at 144, 240, 300, 512, 1023 and 1024 disparities, so that it stands as the yardstick of
tests/test_gpu_generic_ranges.py there; what fsgm_epi_auto_pipeline answers for these ranges; and the limit of plan creation.

The four large frames are wide on purpose: on a narrow one every far sample clamps to the border, no winner lies above 255 and
the comparison would say nothing about the upper range -- so each of them asserts the share of winners >= 256."""
import ctypes

import numpy as np
import pytest

from fsgm_amd import _lib
from fsgm_amd.epi import auto_pipeline
from oracle import pyref
from tests import ref_cases as R

GENERIC = (144, 176, 208, 240, 257, 260, 300, 511, 512, 1000, 1023, 1024)
LARGE = [(97, 31, 300, "axis", 6, 64), (64, 20, 512, "general", 6, 64), (120, 24, 1023, "radial", 100, 200),
         (120, 24, 1024, "general", 6, 64)]
BELOW_256 = [(23, 9, 144, "general", 6, 64), (17, 10, 240, "general", 100, 200)]
FSGM_ERR_UNSUPPORTED = 4


def epi_case(W, H, D, kind, P1, P2):
    """The arguments of calc_cost_sgm for one row of the tables above (shared with the GPU file)."""
    return R._epi(W, H, D, kind, P1, P2, W + D, H)[1]()


@pytest.mark.parametrize("W,H,D,kind,P1,P2", LARGE + BELOW_256)
def test_oracle_equals_reference_at_a_generic_range(oracle, W, H, D, kind, P1, P2):
    """One 4-path call of the reference's compiled calc_cost_sgm each (it is 4-path and sub-pixel), bit for bit."""
    if not pyref.available("calc_cost_sgm"):
        pytest.skip("oracle/_ref/ref_calc_cost_sgm.so is not built (no reference tree on this machine)")
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = a = epi_case(W, H, D, kind, P1, P2)
    ref, printed = pyref.call_calc_cost_sgm(*a)
    want = oracle.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, 4)
    for g, w, n in zip(ref[:2], want, ("bestD", "minC")):
        assert g.dtype == w.dtype and g.shape == w.shape, n
        np.testing.assert_array_equal(g, w, err_msg=n)
    assert not ref[2].any() and not ref[3].any() and printed == ""
    if D > 256:
        # the winning index itself (the reference's bestD has gone through the parabola and the vz conversion), from the
        # oracle's stages, which the lines above have just tied to the reference
        Cv = oracle.epi_cost(I1, I2, D, vMax, pd0, nd, off)
        idx, mc = oracle.epi_wta(oracle.epi_aggregate(Cv, P1, P2, 4), W, H, D, 0)
        np.testing.assert_array_equal(mc, ref[1], err_msg="minC of the staged oracle")
        share = float((idx >= 256).mean())
        print(f"{W}x{H}x{D}: share of winners >= 256 = {share:.3f}, largest {int(idx.max())}")
        assert share >= 0.15, share


@pytest.mark.parametrize("D", GENERIC)
def test_ranges_take_the_generic_kernels_at_every_batch_size(D):
    for W, H in ((1242, 375), (37, 21)):
        for B in (1, 40, 512):
            for paths in (4, 8):
                for P1, P2 in ((6, 64), (100, 200)):
                    for adaptive in (0, 1):
                        assert auto_pipeline(W, H, D, B, paths, P1, P2, adaptive_p2=adaptive) == "generic", (W, H, B, paths, P1, P2, adaptive)


def test_plan_creation_accepts_1024_and_refuses_1025():
    """Without a device a valid shape gets as far as the device check (FSGM_ERR_NO_DEVICE); 1025 is refused before it."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    st = lib.fsgm_epi_plan_create(ctypes.byref(h), 10, 10, 1025, 1, None)
    assert st == FSGM_ERR_UNSUPPORTED and not h.value
    assert b"1025" in lib.fsgm_last_error() and b"1024" in lib.fsgm_last_error()
    st = lib.fsgm_epi_plan_create(ctypes.byref(h), 10, 10, 1024, 1, None)
    if lib.fsgm_device_count() > 0:
        assert st == 0 and h.value
        assert lib.fsgm_epi_plan_kernel_name(h) == b"generic"
        lib.fsgm_epi_plan_destroy(h)
    else:
        assert st == 2 and b"no HIP device" in lib.fsgm_last_error()         # FSGM_ERR_NO_DEVICE: the range itself passed
