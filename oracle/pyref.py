"""ctypes loader of the reference's own MEX code, built into oracle/_ref/ by oracle/Makefile's `ref` target (the four MEX
sources, unmodified, against the stand-in runtime of oracle/refmex/).

TEST INFRASTRUCTURE, beside pyoracle.py: tests/test_oracle_ref_parity.py, tests/golden/make_ref_mex_golden.py and the
reference-direct cases of tests/test_gpu_ref_golden.py use it.  It reads oracle/_ref/ only, never the reference tree.

Conventions are pyoracle's: images (H, W) uint8, maps (2, H, W) / (H, W) float64.  A C-order numpy array (..., H, W) is the
column-major MATLAB array W x H x ... the MEX files expect (they are handed permuted images); scalars go in as 1x1 doubles.
Every call_* returns (outputs, printed): the arrays the mexFunction wrote and the text it passed to mexPrintf.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "_ref")
NAMES = ("calc_cost_sgm", "calc_cost_sgm_ng", "calc_pyd_cost_sgm", "calc_pyd_cost_sgm_ng")
_CLASS = {np.dtype(np.float64): 6, np.dtype(np.uint8): 9, np.dtype(np.uint32): 13}      # mxClassID of refmex/mex.h
_rt = None
_mex = {}


def _path(name):
    return os.path.join(_DIR, f"ref_{name}.so")


def available(name=None):
    """Whether the reference binary for one MEX file (all four when name is None) and the runtime are built."""
    names = NAMES if name is None else (name,)
    return os.path.exists(os.path.join(_DIR, "librefmex.so")) and all(os.path.exists(_path(n)) for n in names)


def _runtime():
    global _rt
    if _rt is None:
        _rt = C.CDLL(os.path.join(_DIR, "librefmex.so"))          # local: tests/mexstub's runtime defines the same mx* names
        _rt.refmex_wrap.restype = C.c_void_p
        _rt.refmex_wrap.argtypes = [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_void_p]
        _rt.refmex_destroy.argtypes = [C.c_void_p]
        _rt.refmex_destroy.restype = None
        _rt.mxGetData.restype = C.c_void_p
        _rt.mxGetData.argtypes = [C.c_void_p]
        _rt.refmex_numel.restype = C.c_size_t
        _rt.refmex_numel.argtypes = [C.c_void_p]
        _rt.refmex_printed.restype = C.c_char_p
    return _rt


def _wrap(a, keep):
    a = np.ascontiguousarray(a)
    keep.append(a)
    dims = a.shape[::-1] if a.ndim >= 2 else (1, 1)
    arr = (C.c_size_t * len(dims))(*dims)
    return _runtime().refmex_wrap(len(dims), arr, _CLASS[a.dtype], a.ctypes.data)


def _scalar(v, keep):
    return _wrap(np.array([float(v)], np.float64), keep)


def _call(name, arrays_and_scalars, outs):
    """mexFunction of ref_<name>.so on the given right-hand sides (numpy arrays, or Python numbers for scalars);
    outs: [(shape, dtype)] of the left-hand sides it creates."""
    rt = _runtime()
    if name not in _mex:
        # deep binding: the object's mx* calls go to the librefmex.so it is linked with, whatever else the process has loaded
        # with global visibility (the gateway tests load tests/mexstub's runtime that way)
        _mex[name] = C.CDLL(_path(name), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        _mex[name].mexFunction.restype = None
    keep = []
    rhs = [_wrap(a, keep) if isinstance(a, np.ndarray) else _scalar(a, keep) for a in arrays_and_scalars]
    prhs = (C.c_void_p * len(rhs))(*rhs)
    plhs = (C.c_void_p * max(len(outs), 1))()
    rt.refmex_clear_printed()
    try:
        _mex[name].mexFunction(C.c_int(len(outs)), plhs, C.c_int(len(rhs)), prhs)
        res = []
        for p, (shape, dt) in zip(plhs, outs):
            n = int(np.prod(shape))
            assert p and rt.refmex_numel(p) == n, f"{name}: output of {rt.refmex_numel(p) if p else None} elements, expected {n}"
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(rt.mxGetData(p))
            res.append(np.frombuffer(buf, dt).reshape(shape).copy())
        printed = rt.refmex_printed().decode()
    finally:
        for p in list(plhs) + rhs:
            if p:
                rt.refmex_destroy(p)
    return tuple(res), printed


def _u8(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.uint8 and a.ndim == 2
    return a


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def call_calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2):
    """((bestD, minC, conf, bestD2), printed).  conf / bestD2 are created by the MEX and left zero: its forward-backward
    check is commented out."""
    I1, I2 = _u8(I1), _u8(I2)
    H, W = I1.shape
    return _call("calc_cost_sgm", [I1, I2, D, vMax, _f64(pd0), _f64(nd), _f64(off), P1, P2],
                 [((H, W), np.uint32), ((H, W), np.uint32), ((H, W), np.uint8), ((H, W), np.uint32)])


def call_calc_pyd_cost_sgm(I1, I2, preMv, rX, rY, rAgg, subpixel, P1, P2, diagonal=1, totalPass=2, adaptiveP2=0):
    """((bestD, minC, mvSub), printed)."""
    I1, I2 = _u8(I1), _u8(I2)
    H, W = I1.shape
    return _call("calc_pyd_cost_sgm", [I1, I2, _f64(preMv), rX, rY, rAgg, subpixel, P1, P2, diagonal, totalPass, adaptiveP2],
                 [((H, W), np.uint32), ((H, W), np.uint32), ((2, H, W), np.float64)])


def call_calc_pyd_cost_sgm_ng(I1, I2, preMv, halfSearchWinSize, aggSize, subpixel, P1, P2):
    """((minC, flow), printed)."""
    I1, I2 = _u8(I1), _u8(I2)
    H, W = I1.shape
    return _call("calc_pyd_cost_sgm_ng", [I1, I2, _f64(preMv), halfSearchWinSize, aggSize, subpixel, P1, P2],
                 [((H, W), np.uint32), ((2, H, W), np.float64)])


def libc_rand_stream(n, seed):
    """n values of libc rand() after srand(seed), drawn from libc itself."""
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(C.c_uint(seed))
    return np.array([libc.rand() for _ in range(n)], np.int32)


def call_calc_cost_sgm_ng(I1, I2, P1, P2, seed=1, preMv=None, halfSearchWinSize=1, aggSize=2, subpixel=0):
    """((minC, flow), printed), with libc srand(seed) right before the call: the MEX draws its candidates from rand().
    preMv and the three scalars after it are read and ignored by the MEX (ng_sgm.m:20 passes zeros, 1, 2, 0)."""
    I1, I2 = _u8(I1), _u8(I2)
    H, W = I1.shape
    preMv = np.zeros((2, H, W)) if preMv is None else _f64(preMv)
    _runtime()
    C.CDLL(None).srand(C.c_uint(seed))
    return _call("calc_cost_sgm_ng", [I1, I2, preMv, halfSearchWinSize, aggSize, subpixel, P1, P2],
                 [((H, W), np.uint32), ((2, H, W), np.float64)])
