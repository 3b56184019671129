"""Rectified stereo with a usable map straight from the device: stereo_sgm's matcher, then the chain of test.m:45-50 --
speckle filter, second-view map, forward-backward check, island removal, scan-line in-fill -- on the rectified geometry
(include/fsgm.h, "Rectified stereo: checked, filtered and filled disparity maps"), and the two new stages on their own.

Maps are (height, width) float64, or a batch (N, height, width), NaN = invalid."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .epi import _d_min, _stereo_params

MAX_WIDTH = 8192                                               # the row kernel's LDS row: 8 * width bytes within 64 KiB
CHAIN_FIELDS = ("speckle_max_diff", "speckle_max_size", "fb_threshold", "island_fraction")


class StereoPPParams(C.Structure):
    _fields_ = [("speckle_max_diff", C.c_double), ("speckle_max_size", C.c_double), ("fb_threshold", C.c_double),
                ("island_fraction", C.c_double), ("in_fill", C.c_int32), ("reserved", C.c_int32 * 7)]


def _bind(lib):
    if getattr(lib, "_stereo_pp_bound", False):
        return
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    sp, opt, pp = C.POINTER(_lib.StereoParams), C.POINTER(_lib.EpiOptions), C.POINTER(StereoPPParams)
    lib.fsgm_stereo_pp_params_default.restype = StereoPPParams
    lib.fsgm_stereo_pp_launch_lds.argtypes = [i32, C.POINTER(C.c_uint64)]
    lib.fsgm_stereo_sgm_pp_host.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, sp, opt, i32, pp, vp, vp, vp, vp, vp]
    lib.fsgm_stereo_sgm_pp_device.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, sp, opt, i32, pp, vp, vp, vp, vp, vp, vp, vp]
    lib.fsgm_stereo_sgm_pp_time.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, sp, opt, i32, pp, i32, i32, C.POINTER(C.c_float)]
    lib.fsgm_stereo_disp_from_first_host.argtypes = [i32, vp, i32, i32, i32, i32, vp, i32]
    lib.fsgm_stereo_disp_from_first_device.argtypes = [i32, vp, i32, i32, i32, i32, vp, i32, vp, vp]
    lib.fsgm_stereo_fb_check_host.argtypes = [i32, vp, vp, i32, i32, i32, i32, f64, vp, vp, i32]
    lib.fsgm_stereo_fb_check_device.argtypes = [i32, vp, vp, i32, i32, i32, i32, f64, vp, vp, i32, vp, vp]
    lib._stereo_pp_bound = True


def _lib_bound():
    lib = _lib.load()
    _bind(lib)
    return lib


def pp_params(lib, in_fill=1, chain=None):
    """fsgm_stereo_pp_params: the defaults with the chain's fields overridden by name (speckle_max_diff, speckle_max_size,
    fb_threshold, island_fraction)"""
    _bind(lib)
    prm = lib.fsgm_stereo_pp_params_default()
    prm.in_fill = int(in_fill)
    for k, v in (chain or {}).items():
        if k not in CHAIN_FIELDS:
            raise TypeError(f"unknown stereo_sgm_pp parameter {k!r}")
        setattr(prm, k, float(v))
    return prm


def launch_lds(width):
    """the dynamic LDS bytes of the row kernel at this width (fsgm_stereo_pp_launch_lds); FsgmError above 8192.  No device."""
    lib = _lib_bound()
    v = C.c_uint64()
    check(lib.fsgm_stereo_pp_launch_lds(int(width), C.byref(v)))
    return int(v.value)


def _images(left, right):
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim not in (2, 3):
        raise TypeError(f"left / right must be uint8 arrays (height, width) or (N, height, width) (got {left.dtype} {left.shape})")
    if right.shape != left.shape:
        raise TypeError(f"right must have left's shape {left.shape} (got {right.shape})")
    if left.ndim == 3 and left.shape[0] == 0:
        raise ValueError("empty batch")
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def stereo_sgm_pp(left, right, dMax, P1=6, P2=64, *, paths=4, subpixel=1, direction=-1, adaptive_p2=0, d_min=0, in_fill=1, device=0,
                  **chain):
    """(disp_pp, disp_checked, disp, minC, disp2) = stereo_sgm_pp(left, right, dMax): stereo_sgm's matcher on the search range
    d_min .. d_min + dMax - 1, then on the device the chain of test.m:45-50 on the candidate-index map: speckle filter,
    second-view map, forward-backward check, island removal and (in_fill=1) scan-line in-fill.  left, right (height, width)
    uint8 or a batch (N, height, width); matcher arguments as stereo_sgm.  Keyword overrides of the chain: speckle_max_diff
    (2), speckle_max_size (100), fb_threshold (2.0), island_fraction (0.1).

    disp_pp float64: the filled true disparities; disp_checked float64: the checked ones, NaN where rejected (its NaN pattern
    is the validity mask); disp int32 (true disparity * 256) and minC uint32: the matcher's raw outputs, as stereo_sgm with
    d_min gives them; disp2 float64: the second-view map, -1 where nothing landed."""
    d_min = _d_min(0 if d_min is None else d_min)
    left, right = _images(left, right)
    if int(dMax) < 1:
        raise ValueError(f"dMax must be >= 1 (got {dMax!r})")
    prm = _stereo_params(paths, subpixel, direction, 0, device)
    lib = _lib_bound()
    pp = pp_params(lib, in_fill, chain)
    opt = _lib.options(adaptive_p2)
    H, W = left.shape[-2:]
    n = 1 if left.ndim == 2 else left.shape[0]
    disp_pp, checked, disp2 = (np.empty(left.shape, np.float64) for _ in range(3))
    disp, minC = np.empty(left.shape, np.int32), np.empty(left.shape, np.uint32)
    check(lib.fsgm_stereo_sgm_pp_host(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt), d_min,
                                      C.byref(pp), ptr(disp_pp), ptr(checked), ptr(disp), ptr(minC), ptr(disp2)))
    return disp_pp, checked, disp, minC, disp2


def stereo_sgm_pp_time(left, right, dMax, P1=6, P2=64, *, paths=4, subpixel=1, direction=-1, adaptive_p2=0, d_min=0, in_fill=1,
                       device=0, warmup=2, iters=10, **chain):
    """(ms of the matcher, ms of the chain, ms of the fused row kernel, ms of the epipolar chain's two generic kernels on
    rectified maps): averages over `iters` warm runs by HIP events (fsgm_stereo_sgm_pp_time)."""
    d_min = _d_min(0 if d_min is None else d_min)
    left, right = _images(left, right)
    prm = _stereo_params(paths, subpixel, direction, 0, device)
    lib = _lib_bound()
    pp = pp_params(lib, in_fill, chain)
    opt = _lib.options(adaptive_p2)
    H, W = left.shape[-2:]
    n = 1 if left.ndim == 2 else left.shape[0]
    ms = (C.c_float * 4)()
    check(lib.fsgm_stereo_sgm_pp_time(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt), d_min,
                                      C.byref(pp), int(warmup), int(iters), ms))
    return tuple(float(v) for v in ms)


def _maps(a, name, shape=None):
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64 or a.ndim not in (2, 3):
        raise TypeError(f"{name} must be a float64 map (height, width) or a batch (N, height, width)")
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}")
    return a


def stereo_disp_from_first(D1, d_min=0, direction=-1, *, device=0):
    """D2 = calc_disp_from_first.m on the rectified geometry: every pixel of D1 (non-negative values or NaN) offers its value
    to the two columns around x + 1 + (d_min + D1) * direction in its own row and the row below; a cell keeps the largest
    offer, -1 where nothing lands.  D1 (height, width) or (N, height, width) float64."""
    lib = _lib_bound()
    D1 = _maps(D1, "D1")
    H, W = D1.shape[-2:]
    D2 = np.empty_like(D1)
    check(lib.fsgm_stereo_disp_from_first_host(1 if D1.ndim == 2 else D1.shape[0], ptr(D1), W, H, _d_min(d_min), int(direction), ptr(D2),
                                               int(device)))
    return D2


def stereo_fb_check(D1, D2=None, d_min=0, direction=-1, thr=2.0, *, device=0, return_second=False):
    """forward_backward_check.m on the rectified geometry: a valid pixel of D1 becomes NaN when its target column
    round(x + 1 + (d_min + D1) * direction) leaves the image, D2 there is -1, or |D1 - D2| > thr.  D2=None: the second-view
    map is made from D1 itself in the same kernel -- the form the chain runs; return_second=True then returns (checked, D2)."""
    lib = _lib_bound()
    D1 = _maps(D1, "D1")
    H, W = D1.shape[-2:]
    if D2 is not None:
        if return_second:
            raise ValueError("return_second needs D2=None")
        D2 = _maps(D2, "D2", D1.shape)
    out = np.empty_like(D1)
    second = np.empty_like(D1) if return_second else None
    check(lib.fsgm_stereo_fb_check_host(1 if D1.ndim == 2 else D1.shape[0], ptr(D1), ptr(D2), W, H, _d_min(d_min), int(direction), float(thr),
                                        ptr(out), ptr(second), int(device)))
    return (out, second) if return_second else out
