"""Generates tests/golden/ref_mex_<file>.npz, one per MEX file, from the REFERENCE's own compiled MEX code (oracle/_ref/ref_*.so,
built by oracle/Makefile from the unmodified sources against the stand-in runtime oracle/refmex/; called through
oracle/pyref.py).  Run in the build container (the reference tree is not on the GPU box), after the build:
    python tests/golden/make_ref_mex_golden.py [MEX file name ...]        (no name: all four)
Each fixture holds data only, as numeric arrays: per case i the inputs (c<i>_I1, c<i>_I2, the hint map c<i>_preMv or the epipolar
maps c<i>_pd0 / _nd / _off, the scalar arguments in MEX order as c<i>_args) and every output the reference wrote (c<i>_out<k>);
`n` is the number of cases.  calc_cost_sgm_ng's c<i>_args ends with the srand seed, and c<i>_rand holds the values libc rand()
returned after that srand (drawn from libc, not from a restatement of it).  Every case runs twice and must repeat itself byte
for byte (which also catches reads of uninitialised memory in the reference); the oracle is not involved."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyref            # noqa: E402
from tests import ref_cases         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def run(name, a):
    if name == "calc_cost_sgm":
        I1, I2, D, vMax, pd0, nd, off, P1, P2 = a
        ins = dict(I1=I1, I2=I2, pd0=pd0, nd=nd, off=off, args=np.array([D, vMax, P1, P2], np.float64))
        call = lambda: pyref.call_calc_cost_sgm(*a)                                     # noqa: E731
    elif name == "calc_cost_sgm_ng":
        I1, I2, P1, P2, seed = a
        H, W = I1.shape
        ins = dict(I1=I1, I2=I2, args=np.array([P1, P2, seed], np.float64), rand=pyref.libc_rand_stream(8 * W * H, seed))
        call = lambda: pyref.call_calc_cost_sgm_ng(*a)                                  # noqa: E731
    else:
        ins = dict(I1=a[0], I2=a[1], preMv=a[2], args=np.array(a[3:], np.float64))
        call = lambda: getattr(pyref, "call_" + name)(*a)                               # noqa: E731
    (outs, printed), (outs2, printed2) = call(), call()
    assert printed == printed2
    for x, y in zip(outs, outs2):
        assert x.tobytes() == y.tobytes(), f"{name}: the reference does not repeat itself"
    return ins, outs


for name in sys.argv[1:] or pyref.NAMES:
    arrays = {}
    cases = ref_cases.golden_cases(name)
    for i, (cid, build) in enumerate(cases):
        ins, outs = run(name, build())
        arrays.update({f"c{i}_{k}": np.ascontiguousarray(v) for k, v in ins.items()})
        arrays.update({f"c{i}_out{k}": v for k, v in enumerate(outs)})
    arrays["n"] = np.array(len(cases), np.int64)
    path = os.path.join(HERE, f"ref_mex_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote ref_mex_{name}.npz: {len(cases)} cases, {os.path.getsize(path)} bytes")
