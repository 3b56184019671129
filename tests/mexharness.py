"""Drives the mexFunction gateways (fsgm_amd/mex/*.mexstub.so) the way MATLAB would, through the
test stub of the MEX API (tests/mexstub).  numpy (H, W) C-order <-> MATLAB W x H column-major.

Arguments of call() / call_full():
  a numpy array         -> an mxArray of its class, dimensions reversed ((n, 2, H, W) is W x H x 2 x n; (H, 0) is 0 x H)
  a Python number       -> a 1x1 double (what a MATLAB literal is)
  a numpy scalar        -> a 1x1 array of its class: np.float32(0.3) is single(0.3), np.int32(16) is int32(16), np.bool_(1) is
                           logical(1), np.float64(x) a double
  Arr(data, dims)       -> the data under an explicit MATLAB dimension list (W x H x 1, 1 x 2, 0 x 0, ...)
"""
import ctypes as C
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEXDIR = os.path.join(ROOT, "fsgm_amd", "mex")
_CLS = {np.dtype(np.float64): 6, np.dtype(np.uint8): 9, np.dtype(np.uint32): 13,
        np.dtype(np.bool_): 3, np.dtype(np.float32): 7, np.dtype(np.int8): 8, np.dtype(np.int16): 10, np.dtype(np.uint16): 11,
        np.dtype(np.int32): 12, np.dtype(np.int64): 14, np.dtype(np.uint64): 15}
_DT = {c: dt.type for dt, c in _CLS.items()}
_stub = None


class MexError(RuntimeError):
    """mexErrMsgIdAndTxt was called.  live_before / live_after: the stub's count of live mxArrays before the inputs were made
    and right after the call came back (inputs still alive): live_after - live_before - nrhs arrays leaked."""
    def __init__(self, ident, msg, live_before=0, live_after=0, nrhs=0):
        super().__init__(f"{ident}: {msg}")
        self.ident = ident
        self.msg = msg
        self.live_before, self.live_after, self.nrhs = live_before, live_after, nrhs

    @property
    def leaked(self):
        return self.live_after - self.live_before - self.nrhs


class Arr:
    """data (any numpy array; its class is the mxArray's) under the MATLAB dimension list dims, column-major: the C-order
    bytes of data are the array's memory as they stand."""
    def __init__(self, data, dims):
        self.data = np.ascontiguousarray(data)
        self.dims = tuple(int(d) for d in dims)
        assert int(np.prod(self.dims)) == self.data.size, (self.dims, self.data.shape)


class Result:
    """What call_full() saw: outs (numpy, dimensions reversed), out_dims (the MATLAB dimension lists), printed, inputs_after (the
    input mxArrays read back after the call), live_before / live_after (see MexError; live_after counts inputs and outputs)."""
    def __init__(self, outs, out_dims, printed, inputs_after, live_before, live_after):
        self.outs, self.out_dims, self.printed, self.inputs_after = outs, out_dims, printed, inputs_after
        self.live_before, self.live_after = live_before, live_after


def stub():
    global _stub
    if _stub is None:
        s = C.CDLL(os.path.join(MEXDIR, "libmexstub.so"), mode=C.RTLD_GLOBAL)
        s.mxCreateNumericArray.restype = C.c_void_p
        s.mxCreateNumericArray.argtypes = [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int]
        s.mxCreateDoubleScalar.restype = C.c_void_p
        s.mxCreateDoubleScalar.argtypes = [C.c_double]
        s.mxDestroyArray.argtypes = [C.c_void_p]
        s.mxGetData.restype = C.c_void_p
        s.mxGetData.argtypes = [C.c_void_p]
        s.mxGetScalar.restype = C.c_double
        s.mxGetScalar.argtypes = [C.c_void_p]
        s.mxGetNumberOfDimensions.restype = C.c_size_t
        s.mxGetNumberOfDimensions.argtypes = [C.c_void_p]
        s.mxGetDimensions.restype = C.POINTER(C.c_size_t)
        s.mxGetDimensions.argtypes = [C.c_void_p]
        s.mxGetClassID.argtypes = [C.c_void_p]
        s.mexstub_call.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
        s.mexstub_last_error_id.restype = C.c_char_p
        s.mexstub_last_error_msg.restype = C.c_char_p
        s.mexstub_printed.restype = C.c_char_p
        s.mexstub_live_arrays.restype = C.c_long
        _stub = s
    return _stub


def live_arrays():
    """mxArrays the stub has created and not yet destroyed"""
    return int(stub().mexstub_live_arrays())


def _make(data, dims):
    s = stub()
    arr = (C.c_size_t * len(dims))(*dims)
    m = s.mxCreateNumericArray(len(dims), arr, _CLS[data.dtype], 0)
    if data.nbytes:
        C.memmove(s.mxGetData(m), data.ctypes.data, data.nbytes)
    return m


def to_mx(a):
    s = stub()
    if isinstance(a, Arr):
        return _make(a.data, a.dims)
    if isinstance(a, np.generic) and a.dtype != np.float64:           # single(0.3), int32(16), logical(1): a 1x1 of that class
        return _make(np.array([a]), (1, 1))
    if np.isscalar(a):
        return s.mxCreateDoubleScalar(float(a))
    a = np.ascontiguousarray(a)
    return _make(a, tuple(reversed(a.shape)))              # C-order (.., H, W) -> MATLAB W x H x ..


def dims_of(m):
    s = stub()
    return tuple(int(s.mxGetDimensions(m)[i]) for i in range(s.mxGetNumberOfDimensions(m)))


def from_mx(m):
    s = stub()
    dims = dims_of(m)
    dt = _DT[s.mxGetClassID(m)]
    n = int(np.prod(dims))
    out = np.empty(tuple(reversed(dims)), dt)
    if n:
        C.memmove(out.ctypes.data, s.mxGetData(m), n * np.dtype(dt).itemsize)
    return out


def scalar_of(a):
    """what mxGetScalar returns for the argument a (see the module docstring)"""
    s = stub()
    m = to_mx(a)
    try:
        return float(s.mxGetScalar(m))
    finally:
        s.mxDestroyArray(m)


def sent(a):
    """the mxArray made from the argument a, read back: what inputs_after holds for an input the call left alone"""
    m = to_mx(a)
    try:
        return from_mx(m)
    finally:
        stub().mxDestroyArray(m)


def call_full(name, nlhs, *args):
    """mexFunction of the gateway `name` with nlhs outputs asked for; a Result, or MexError on mexErrMsgIdAndTxt.  Inputs and
    outputs are destroyed before it returns: the stub's live count is back at live_before unless the gateway leaked."""
    s = stub()
    lib = C.CDLL(os.path.join(MEXDIR, f"{name}.mexstub.so"))
    fn = C.cast(lib.mexFunction, C.c_void_p)
    live_before = live_arrays()
    prhs = (C.c_void_p * max(1, len(args)))(*[to_mx(a) for a in args])
    plhs = (C.c_void_p * max(1, nlhs, 20))()
    rc = s.mexstub_call(fn, nlhs, plhs, len(args), prhs)
    live_after = live_arrays()
    printed = s.mexstub_printed().decode()
    n_out = max(1, nlhs)                                   # MATLAB takes plhs[0] (ans) even at nlhs = 0
    try:
        if rc:
            raise MexError(s.mexstub_last_error_id().decode(), s.mexstub_last_error_msg().decode(), live_before, live_after,
                           len(args))
        assert all(plhs[i] for i in range(n_out)), f"{name}: an output asked for was not created"
        outs = [from_mx(plhs[i]) for i in range(n_out)]
        out_dims = [dims_of(plhs[i]) for i in range(n_out)]
        inputs_after = [from_mx(prhs[i]) for i in range(len(args))]
    finally:
        for i in range(len(args)):
            s.mxDestroyArray(prhs[i])
        if not rc:
            for i in range(n_out):
                s.mxDestroyArray(plhs[i])
    return Result(outs, out_dims, printed, inputs_after, live_before, live_after)


def call(name, nlhs, *args):
    """outputs = call('calc_cost_sgm', 2, I1, I2, 64, 0.3, ...) ; raises MexError on mexErrMsgIdAndTxt"""
    r = call_full(name, nlhs, *args)
    return r.outs, r.printed
