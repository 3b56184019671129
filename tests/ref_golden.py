"""Reader of the reference-written fixtures tests/golden/ref_mex_<file>.npz (tests/golden/make_ref_mex_golden.py): per case the
inputs the reference's compiled mexFunction was given and every output it wrote."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("calc_cost_sgm", "calc_cost_sgm_ng", "calc_pyd_cost_sgm", "calc_pyd_cost_sgm_ng")
COUNTS = {"calc_cost_sgm": 11, "calc_cost_sgm_ng": 10, "calc_pyd_cost_sgm": 21, "calc_pyd_cost_sgm_ng": 12}
_INPUTS = ("I1", "I2", "preMv", "pd0", "nd", "off", "args", "rand")
_cache = {}


def case(name, i):
    """dict of the inputs present for this MEX file plus outs = [out0, out1, ...]."""
    if name not in _cache:
        with np.load(os.path.join(GOLD, f"ref_mex_{name}.npz"), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    z = _cache[name]
    assert int(z["n"]) == COUNTS[name]
    c = {k: z[f"c{i}_{k}"] for k in _INPUTS if f"c{i}_{k}" in z}
    c["outs"] = [z[f"c{i}_out{k}"] for k in range(8) if f"c{i}_out{k}" in z]
    return c


def ids(name):
    return [(name, i) for i in range(COUNTS[name])]


def ints(args):
    return [int(v) for v in args]
