"""The packed line kernels' disparity ranges beyond 16 << k (agg_line_split, epi_lines.hip: 48, 96, 192 as 12 costs a lane; 80,
160 as 20; 112, 224 as 28), as far as no device is needed: what fsgm_epi_auto_pipeline answers for them, that every other range
keeps its answer, and the CPU oracle against the reference's own compiled code at two of the new ranges, so that the oracle
stands as the yardstick of tests/test_gpu_line_splits.py there."""
import ast
import inspect
import textwrap

import numpy as np
import pytest

from fsgm_amd.epi import auto_pipeline
from oracle import pyref
from tests import ref_cases as R

SPLITS = (48, 80, 96, 112, 160, 192, 224)


@pytest.mark.parametrize("adaptive", (0, 1))
@pytest.mark.parametrize("D", SPLITS)
def test_new_ranges_take_the_packed_line_kernels_at_every_batch_size(D, adaptive):
    for W, H in ((1242, 375), (37, 21)):
        for B in (1, 40, 512):
            for paths in (4, 8):
                assert auto_pipeline(W, H, D, B, paths, 6, 64, adaptive_p2=adaptive) == "packed16/nowrap", (W, H, B, paths)
                assert auto_pipeline(W, H, D, B, paths, 100, 200, adaptive_p2=adaptive) == "packed16/wrap", (W, H, B, paths)


@pytest.mark.parametrize("D", (144, 176, 208, 240, 100, 72, 20))
def test_other_ranges_stay_generic(D):
    for B in (1, 40, 512):
        for paths in (4, 8):
            for P1, P2 in ((6, 64), (100, 200)):
                for adaptive in (0, 1):
                    assert auto_pipeline(1242, 375, D, B, paths, P1, P2, adaptive_p2=adaptive) == "generic", (B, paths, P1, P2, adaptive)


def _kitti_table():
    """The (paths, batch, name) list of tests/test_capi_cpu.py::test_auto_mode_table, read from that function's own source."""
    from tests import test_capi_cpu as T
    tree = ast.parse(textwrap.dedent(inspect.getsource(T.test_auto_mode_table)))
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "kitti":
            return ast.literal_eval(node.value)
    raise LookupError("test_auto_mode_table: no list named kitti")


def test_the_answers_at_128_disparities_are_what_they_were():
    table = _kitti_table()
    assert len(table) >= 10 and {name for _, _, name in table} > {"packed16/nowrap"}       # the table names fused pipelines too
    for paths, B, name in table:
        assert auto_pipeline(1242, 375, 128, B, paths, 6, 64) == name, (paths, B)


@pytest.mark.parametrize("W,H,D,P1,P2", [(37, 21, 48, 6, 64), (26, 13, 192, 100, 200)])
def test_oracle_equals_reference_at_a_new_range(oracle, W, H, D, P1, P2):
    """One 4-path call of the reference's compiled calc_cost_sgm each (it is 4-path and sub-pixel), bit for bit."""
    if not pyref.available("calc_cost_sgm"):
        pytest.skip("oracle/_ref/ref_calc_cost_sgm.so is not built (no reference tree on this machine)")
    I1, I2, D, vMax, pd0, nd, off, P1, P2 = a = R._epi(W, H, D, "general", P1, P2, W + D, H)[1]()
    ref, printed = pyref.call_calc_cost_sgm(*a)
    want = oracle.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, 4)
    for g, w, n in zip(ref[:2], want, ("bestD", "minC")):
        assert g.dtype == w.dtype and g.shape == w.shape, n
        np.testing.assert_array_equal(g, w, err_msg=n)
    assert not ref[2].any() and not ref[3].any() and printed == ""
