"""The search windows the calc_pyd_cost_sgm path accepts, as limits, and the dynamic LDS its launches ask for -- all of it
without a device: fsgm_pyd_plan_create checks its window before it touches one, and fsgm_pyd_launch_lds (pyd.launch_lds) evaluates
the launchers' own expressions (fsgm_amd/csrc/pyd_kernels.h) for a window and an aggregation radius."""
import ctypes as C

import numpy as np
import pytest

from fsgm_amd import FsgmError, PydPlan, calc_pyd_cost_sgm, pyd
from tests import ref_cases as R

UNSUPPORTED, NO_DEVICE = 4, 2
LDS_LIMIT = 65536            # what a workgroup may ask for without an opt-in
PATCH_LIMIT = 49152          # the cost stage leaves the patch kernel above this (PYD_PATCH_LDS_MAX)


def _accepted(call):
    """The call got past the argument checks: it succeeds, or fails for want of a device (tests/test_capi_cpu.py)."""
    try:
        res = call()
    except FsgmError as e:
        assert e.status == NO_DEVICE and "no HIP device" in str(e), e
        return
    if hasattr(res, "close"):
        res.close()


REFUSED = [(32, 0, "search window side exceeds 64"), (0, 32, "search window side exceeds 64"),
           (32, 32, "search window side exceeds 64"), (16, 16, "search window 1089 candidates exceeds 1024"),
           (31, 8, "search window 1071 candidates exceeds 1024")]


@pytest.mark.parametrize("rX,rY,msg", REFUSED)
def test_windows_beyond_the_limits_are_refused_before_a_device_is_touched(rX, rY, msg):
    I1 = np.zeros((4, 5), np.uint8)
    mv = np.zeros((2, 4, 5))
    calls = (lambda: PydPlan(5, 4, 5, 4, rX, rY, 2),
             lambda: calc_pyd_cost_sgm(I1, I1, mv, rX, rY, 2, 1, 6, 32, 1, 2, 0),
             lambda: pyd.launch_lds(rX, rY, 2))
    for call in calls:
        with pytest.raises(FsgmError) as ei:
            call()
        assert ei.value.status == UNSUPPORTED and msg in str(ei.value)


@pytest.mark.parametrize("rX,rY", [(15, 16), (16, 15), (31, 7), (7, 31), (31, 0), (0, 31), (0, 0)])
def test_the_largest_windows_pass_the_argument_checks(rX, rY):
    I1 = np.zeros((4, 5), np.uint8)
    mv = np.zeros((2, 4, 5))
    _accepted(lambda: PydPlan(5, 4, 5, 4, rX, rY, 2))
    _accepted(lambda: calc_pyd_cost_sgm(I1, I1, mv, rX, rY, 2, 1, 6, 32, 1, 2, 0))
    assert pyd.launch_lds(rX, rY, 2)["agg_lds"] > 0


def test_launch_lds_argument_checks():
    lib = pyd._lib.load()
    pyd._bind(lib)
    k, v = C.c_int32(), C.c_uint64()
    assert lib.fsgm_pyd_launch_lds(1, 1, 1, None, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == 1       # FSGM_ERR_INVALID
    assert lib.fsgm_pyd_launch_lds(-1, 1, 1, C.byref(k), C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == 1
    assert lib.fsgm_pyd_launch_lds(1, 1, -1, C.byref(k), C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == 1


@pytest.fixture(scope="module")
def table():
    """launch_lds for every accepted window and aggregation radius 0..40; every other window up to half size 33 is refused."""
    t = {}
    for rX in range(34):
        for rY in range(34):
            ok = 2 * rX + 1 <= 64 and 2 * rY + 1 <= 64 and (2 * rX + 1) * (2 * rY + 1) <= 1024
            if not ok:
                with pytest.raises(FsgmError) as ei:
                    pyd.launch_lds(rX, rY, 0)
                assert ei.value.status == UNSUPPORTED
                continue
            for rAgg in range(41):
                t[rX, rY, rAgg] = pyd.launch_lds(rX, rY, rAgg)
    return t


def test_no_accepted_window_asks_for_more_than_64_kib(table):
    assert len(table) == 41 * len({k[:2] for k in table}) and len({k[:2] for k in table}) > 300
    for key, r in table.items():
        assert max(r["cost_lds"], r["agg_lds"], r["rows_agg_lds"]) <= LDS_LIMIT, key


def test_the_cost_stage_leaves_the_patch_kernel_exactly_above_48_kib(table):
    for (rX, rY, rAgg), r in table.items():
        rows = rX <= 5 and rY <= 5 and rAgg <= 2               # the row-packed layout's windows, its kernel's radii
        want = "rows" if rows else "candidate" if r["patch_lds"] > PATCH_LIMIT else "patch"
        assert r["cost_kernel"] == want, (rX, rY, rAgg)
        # (the row-packed kernel's request goes by Sx alone: pixels a wave, times a slot of 299 dwords, times 4 waves)
        rows_lds = {1: 38272, 3: 38272, 5: 38272, 7: 38272, 9: 33488, 11: 23920}
        assert r["cost_lds"] == (0 if want == "candidate" else r["patch_lds"] if want == "patch" else rows_lds[2 * rX + 1])
        assert (r["rows_agg_lds"] > 0) == (rX <= 5 and rY <= 5)
    # the pair of cases tests/test_gpu_pyd_windows.py runs: the smallest radius at which any window takes the per-candidate kernel,
    # the window there with the fewest candidates, and the same window one radius below
    fallback = [k for k, r in table.items() if r["cost_kernel"] == "candidate"]
    rmin = min(k[2] for k in fallback)
    first = min((k for k in fallback if k[2] == rmin), key=lambda k: ((2 * k[0] + 1) * (2 * k[1] + 1), k))
    assert first == R.COST_FALLBACK
    assert R.COST_LAST_PATCH == first[:2] + (rmin - 1,) and table[R.COST_LAST_PATCH]["cost_kernel"] == "patch"
    at_bound = table[R.COST_PATCH_AT_BOUND]
    assert at_bound["cost_kernel"] == "patch" and at_bound["patch_lds"] == PATCH_LIMIT
    # its r <= 2 branch is out of reach: no accepted window leaves the patch kernel there
    assert all(r["patch_lds"] <= PATCH_LIMIT for k, r in table.items() if k[2] <= 2)


def test_the_largest_requests_are_pinned(table):
    agg = {k[:2]: r["agg_lds"] for k, r in table.items()}
    top = max(agg.values())
    assert top == 61664 and sorted(k for k, v in agg.items() if v == top) == [(8, 29), (29, 8)]      # 17x59 and 59x17
    assert agg[31, 7] == agg[7, 31] == 60448                                                        # 63x15
    assert agg[15, 16] == 58464 and agg[8, 8] == 25376 and agg[0, 0] == 5920      # 4 * (2 * (Sx + 10) * (Sy + 10) + 128) * 4
    patch = max(r["cost_lds"] for r in table.values() if r["cost_kernel"] == "patch")
    assert patch == PATCH_LIMIT                                   # some window sits on the bound itself (and takes the patch kernel)
    assert {r["rows_agg_lds"] for r in table.values()} == {0, 28672}
    assert max(r["cost_lds"] for r in table.values() if r["cost_kernel"] == "rows") == 38272
