"""torch tensors on the GPU in, torch tensors on the GPU out, ordered on the caller's current stream: the device-pointer entry
points of include/fsgm.h ("Device-pointer entry points") as torch custom ops and friendly wrappers.

    import torch                                   # first: the library must bind to torch's HIP runtime
    from fsgm_amd import torch_ops
    bestD, minC = torch_ops.calc_cost_sgm(I1, I2, 128, 0.3, pd0, nd, off, 6, 64, paths=8)   # cuda tensors

No host<->device copy and no host wait once a plan for the shape exists: the work is queued behind what the current stream
already holds, and what is queued on that stream afterwards runs after it.  Ops registered: fsgm::calc_cost_sgm,
fsgm::calc_cost_sgm_linear, fsgm::stereo_sgm, fsgm::stereo_sgm_range, fsgm::sgm (a caller's cost volumes; status also
FSGM_ERR_INVALID when a cost was above the declared bound), fsgm::sgm2d (the 2-D matcher on a caller's volumes; the same status),
fsgm::epipolar_sgm_of, fsgm::pyramidal_sgm, fsgm::pyramidal_sgm_ng, fsgm::epipolar_flow_pp, fsgm::pyramidal_flow_pp (each also returns a 0-d int32
status tensor: 0, or FSGM_ERR_HIP when an aggregation hand-off gave up; check=True in the wrappers synchronises and raises
on it), fsgm::epi_postprocess (status FSGM_ERR_INVALID when a D1 value is negative), fsgm::vmf and fsgm::flow_fb_check; for rectified
stereo fsgm::stereo_sgm_pp (the matcher and the chain of test.m:45-50) and fsgm::stereo_fb_check (status as fsgm::epi_postprocess),
fsgm::stereo_sgm_ru (fsgm::stereo_sgm_range with the runner-up cost minC2 after minC) and fsgm::uniqueness_filter (status always 0);
fsgm::sgm_ru and fsgm::sgm2d_ru (fsgm::sgm / fsgm::sgm2d with minC2 after minC) and fsgm::uniqueness_filter_planes (a map or a
two-plane flow; status always 0); fsgm::pyramidal_sgm_ru and fsgm::pyramidal_sgm_ng_ru (the pyramids with level 1's minC2 after
minC) and fsgm::pyramidal_flow_pp_u (fsgm::pyramidal_flow_pp with a uniqueness ratio ahead of the chain and minC2 after minC);
fsgm::sgm_exact (fsgm::sgm with exact path arithmetic, fsgm_sgm_device_exact: the same arguments and outputs),
fsgm::sgm2d_exact (fsgm::sgm2d_ru with exact path arithmetic, fsgm_sgm2d_device_exact: a runner_up flag added, minC2 empty without it);
fsgm::pyramidal_sgm_lm, fsgm::pyramidal_sgm_ng_lm and fsgm::pyramidal_flow_pp_lm (the _ru / _u ops with the median between levels:
a level_median argument, minC2 empty when not asked for) and fsgm::flow_level_hints (the hint map of the next finer level).
In a namespace of their own, fsgm_float::sgm and fsgm_float::sgm2d: the sgm and sgm2d families on float32 / float16 / bfloat16
volumes, quantised to bytes in the pass that brings them into the plan (runner_up and exact are flags; sgm_float, sgm2d_float).

One process must hold one HIP runtime.  torch brings its own libamdhip64; libfsgm_hip.so binds to it by soname when torch is
imported first.  When the library was loaded first, torch afterwards maps a second runtime, and a stream or pointer of one
is meaningless to the other: importing this module then raises ImportError.
"""
import torch  # noqa: I001 -- first, before the library: its HIP runtime is the one libfsgm_hip.so must bind to

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _lib
from ._lib import EpiIn, EpiOut, EpiOptions, EpiParams, FsgmError, StereoParams
from .epi import EpiGeometry, _d_min, _params as _epi_params, _stereo_params
from .post import _bind as _bind_post
from .stereo_pp import CHAIN_FIELDS as STEREO_PP_FIELDS, _bind as _bind_stereo_pp, pp_params as _stereo_pp_params
from .sgm import _bind as _bind_sgm, arith_exact as _arith_exact, cost_format as _cost_format, layout_code as _layout_code, params as _sgm_params, shape_of as _sgm_shape
from .view2 import bind as _bind_view2, params as _view2_params
from .sgm2d import _bind as _bind_sgm2d, arith_exact as _arith2d_exact, layout_code as _layout2d_code, params as _sgm2d_params, shape_of as _sgm2d_shape, LAYOUTS as _LAYOUTS2D
from .pyramid import (PyramidParams, NgPyramidParams, FLOW_PP_FIELDS, MATCHERS, _bind as _bind_pyramid, _bind_flow_pp, _bind_ng,
                      uniqueness_ratio_of as _uniqueness_ratio_of, level_median_of as _level_median_of)

FSGM_ERR_INVALID, FSGM_ERR_HIP = 1, 2


def hip_runtimes():
    """The distinct libamdhip64 files mapped into this process (/proc/self/maps)."""
    files = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in parts[5].rsplit("/", 1)[-1]:
                files.add(parts[5].strip())
    return sorted(files)


_L = _lib.load()
_runtimes = hip_runtimes()
if len(_runtimes) != 1:
    raise ImportError(
        "fsgm_amd.torch_ops needs one HIP runtime in the process, found %d: %s.  libfsgm_hip.so was loaded before torch "
        "(e.g. by fsgm_amd.load_library() or a compute call), so torch brought a second runtime whose streams and pointers the "
        "library cannot use.  Import torch (or fsgm_amd.torch_ops) before anything that loads libfsgm_hip.so."
        % (len(_runtimes), ", ".join(_runtimes) or "none"))

_vp, _i32 = C.c_void_p, C.c_int32
_bind_pyramid(_L)
_bind_ng(_L)
_bind_post(_L)
_bind_flow_pp(_L)
_bind_stereo_pp(_L)
_bind_sgm(_L)
_bind_sgm2d(_L)
if hasattr(_L, "fsgm_sgm_view2_dptr"):                          # (an older build behind FSGM_LIB_PATH has none)
    _bind_view2(_L)
_L.fsgm_calc_cost_sgm_device.argtypes = [_i32, C.POINTER(EpiIn), C.POINTER(EpiOut), C.POINTER(EpiParams), _vp, _vp]
_L.fsgm_calc_cost_sgm_linear_device.argtypes = [_i32, C.POINTER(EpiIn), C.POINTER(EpiOut), C.POINTER(EpiParams), _vp, _vp]
_L.fsgm_stereo_sgm_device.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(StereoParams), _vp, _vp, _vp, _vp, _vp, _vp]
_opt = C.POINTER(EpiOptions)
_L.fsgm_calc_cost_sgm_device_opts.argtypes = [_i32, C.POINTER(EpiIn), C.POINTER(EpiOut), C.POINTER(EpiParams), _opt, _vp, _vp]
_L.fsgm_calc_cost_sgm_linear_device_opts.argtypes = [_i32, C.POINTER(EpiIn), C.POINTER(EpiOut), C.POINTER(EpiParams), _opt, _vp, _vp]
_L.fsgm_stereo_sgm_device_opts.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(StereoParams), _opt, _vp, _vp, _vp, _vp,
                                           _vp, _vp]
_L.fsgm_stereo_sgm_device_range.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(StereoParams), _opt, _i32, _vp, _vp, _vp,
                                            _vp, _vp, _vp]
_L.fsgm_epi_plan_run_device.argtypes = [_vp, _i32, C.POINTER(EpiIn), C.POINTER(EpiOut), _vp, _vp]
_L.fsgm_epipolar_sgm_of_device.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(EpiGeometry), _i32, C.c_double,
                                           C.POINTER(EpiParams), _vp, _vp, _vp, _vp]
_L.fsgm_epipolar_flow_pp_device.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(EpiGeometry), _i32, C.c_double,
                                             C.POINTER(EpiParams), _vp, _vp, _vp, _vp, _vp, _vp]
_L.fsgm_pyramidal_sgm_device.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(PyramidParams), _vp, _vp, _vp, _vp]
_L.fsgm_pyramidal_sgm_ng_device.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(NgPyramidParams), _vp, _vp, _vp, _vp]
if hasattr(_L, "fsgm_pyramidal_sgm_device_ru"):                  # (an older build behind FSGM_LIB_PATH has neither)
    _L.fsgm_pyramidal_sgm_device_ru.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(PyramidParams), _vp, _vp, _vp, _vp, _vp]
    _L.fsgm_pyramidal_sgm_ng_device_ru.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(NgPyramidParams), _vp, _vp, _vp, _vp, _vp]
if hasattr(_L, "fsgm_pyramidal_sgm_device_lm"):
    _L.fsgm_pyramidal_sgm_device_lm.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(PyramidParams), _i32, _vp, _vp, _vp, _vp, _vp]
    _L.fsgm_pyramidal_sgm_ng_device_lm.argtypes = [_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(NgPyramidParams), _i32, _vp, _vp, _vp, _vp, _vp]
    _L.fsgm_flow_level_hints_device.argtypes = [_i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp]

# the overridable fields of the pyramids' parameter structs, in the order the ops take them
PYRAMID_FIELDS = ("P1", "P2", "aggHalfWinSize", "verSearchHalfWinSize", "horSearchHalfWinSize", "enableDiagonal", "totalPass", "adaptiveP2")
NG_PYRAMID_FIELDS = ("P1", "P2", "halfSearchWinSize", "aggSize", "subPixelRefine")
GEOMETRY_NUMBERS = 21            # F (9), H (9), epipole (2), direction (1) per frame


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ready(t):
    """t itself when it is contiguous and aligned on its element size, else a contiguous copy (on the current stream)."""
    if t.is_contiguous() and t.data_ptr() % t.element_size() == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _call(dev, fn, *args):
    with torch.cuda.device(dev):                  # the library sets the HIP device of the calling thread: give it back
        _lib.check(fn(*args))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _u32(shape, dev):
    return torch.empty(shape, dtype=torch.uint32, device=dev)


def _status(dev):
    return torch.empty((), dtype=torch.int32, device=dev)


def _f64(shape, dev):
    return torch.empty(shape, dtype=torch.float64, device=dev)


def _geometries(geometry, N):
    """N fsgm_epi_geometry structs from the flat list of the ops (GEOMETRY_NUMBERS per frame)."""
    if len(geometry) != N * GEOMETRY_NUMBERS:
        raise ValueError(f"geometry must hold {GEOMETRY_NUMBERS} numbers per frame ({N * GEOMETRY_NUMBERS}), got {len(geometry)}")
    g = (EpiGeometry * N)()
    for f in range(N):
        v = geometry[f * GEOMETRY_NUMBERS:(f + 1) * GEOMETRY_NUMBERS]
        g[f].F[:] = [float(x) for x in v[0:9]]
        g[f].H[:] = [float(x) for x in v[9:18]]
        g[f].epipole[:] = [float(v[18]), float(v[19])]
        g[f].direction = int(v[20] != 0)
    return g


# ---------------------------------------------------------------------------------------------
# custom ops: every tensor argument is batched (leading N) and on one GPU; outputs freshly allocated there.  Each op's
# outputs are stated once, in an _*_outputs function of the input shapes and flags that its body and its fake both call.
# The ops of one family (a matcher and its _ru / _exact / _u / _lm forms) share one body, an _*_run function that takes the C
# entry: an op function carries the schema -- torch derives it from the annotated signature -- names its own entry and says how
# the entry treats the runner-up cost, `minC2`: None -- the entry has no such argument and the op no such output; True -- a full
# map after minC; False -- the entry is handed NULL there and the op returns an empty (0,) placeholder.  An entry is looked up
# when its op runs, so a call with the newer switches off touches no newer symbol (an older build behind FSGM_LIB_PATH).
# ---------------------------------------------------------------------------------------------
def _frames(t):
    """(N, H, W, device) of a batch of maps (N, H, W) or images (N, H, W) / (N, 3, H, W)."""
    return t.shape[0], t.shape[-2], t.shape[-1], t.device


def _minC2_output(minC, minC2):
    """the minC2 slot of an op's outputs, as a tuple to splice in after minC: nothing, a map like minC, or the placeholder"""
    if minC2 is None:
        return ()
    return (torch.empty_like(minC) if minC2 else _u32((0,), minC.device),)


def _minC2_arg(slot, minC2):
    """the same slot as the C entry's arguments: nothing, the map's address, or NULL"""
    return tuple(_p(t) if minC2 else None for t in slot)


def _fb_outputs(N, H, W, fb_check, dev, dtype=torch.uint32):
    """(conf, the second view's map of `dtype`): empty (0,) placeholders without fb_check."""
    shape = (N, H, W) if fb_check else (0,)
    return torch.empty(shape, dtype=torch.uint8, device=dev), torch.empty(shape, dtype=dtype, device=dev)


def _matcher_outputs(I1, fb_check, dtype=torch.uint32):
    """(bestD of `dtype`, minC, conf, bestD2 of `dtype`, status) of the 1-D matchers."""
    N, H, W, dev = _frames(I1)
    return (torch.empty((N, H, W), dtype=dtype, device=dev), _u32((N, H, W), dev)) + _fb_outputs(N, H, W, fb_check, dev, dtype) + (_status(dev),)


def _epi_structs(I1, I2, pd0, nd, off, W, H, dMax, vMax, P1, P2, bestD, minC, conf=None, bestD2=None):
    """fsgm_epi_in / fsgm_epi_out over these tensors (off, conf, bestD2 may be None)."""
    e, o = EpiIn(), EpiOut()
    e.I1, e.I2, e.width, e.height, e.dMax, e.vMax = _p(I1), _p(I2), W, H, int(dMax), float(vMax)
    e.pixelPosD0, e.normDir, e.offset, e.P1, e.P2 = _p(pd0), _p(nd), _p(off), int(P1), int(P2)
    o.bestD, o.minC, o.conf, o.bestD2 = _p(bestD), _p(minC), _p(conf), _p(bestD2)
    return e, o


def _calc_cost_sgm_run(fn, I1, I2, pd0, nd, off, dMax, vMax, P1, P2, paths, subpixel, vz_to_disp, fb_check, adaptive_p2):
    N, H, W, dev = _frames(I1)
    I1, I2, pd0, nd = (_ready(t) for t in (I1, I2, pd0, nd))
    off = None if off is None else _ready(off)
    bestD, minC, conf, bestD2, status = _matcher_outputs(I1, fb_check)
    e, o = _epi_structs(I1, I2, pd0, nd, off, W, H, dMax, vMax, P1, P2, bestD, minC, conf if fb_check else None,
                        bestD2 if fb_check else None)
    prm = _epi_params(paths, subpixel, vz_to_disp, dev.index, fb_check)
    opt = _lib.options(adaptive_p2)
    _call(dev, fn, N, C.byref(e), C.byref(o), C.byref(prm), C.byref(opt), _stream(dev), _p(status))
    return bestD, minC, conf, bestD2, status


@torch.library.custom_op("fsgm::calc_cost_sgm", mutates_args=())
def _calc_cost_sgm_op(I1: torch.Tensor, I2: torch.Tensor, pd0: torch.Tensor, nd: torch.Tensor, off: torch.Tensor, dMax: int,
                      vMax: float, P1: int, P2: int, paths: int, subpixel: int, vz_to_disp: int,
                      fb_check: int, adaptive_p2: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _calc_cost_sgm_run(_L.fsgm_calc_cost_sgm_device_opts, I1, I2, pd0, nd, off, dMax, vMax, P1, P2, paths, subpixel, vz_to_disp,
                              fb_check, adaptive_p2)


@_calc_cost_sgm_op.register_fake
def _(I1, I2, pd0, nd, off, dMax, vMax, P1, P2, paths, subpixel, vz_to_disp, fb_check, adaptive_p2=0):
    return _matcher_outputs(I1, fb_check)


@torch.library.custom_op("fsgm::calc_cost_sgm_linear", mutates_args=())
def _calc_cost_sgm_linear_op(I1: torch.Tensor, I2: torch.Tensor, pd0: torch.Tensor, nd: torch.Tensor, dMax: int, P1: int, P2: int,
                             paths: int, subpixel: int,
                             fb_check: int, adaptive_p2: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _calc_cost_sgm_run(_L.fsgm_calc_cost_sgm_linear_device_opts, I1, I2, pd0, nd, None, dMax, 0.0, P1, P2, paths, subpixel, 0,
                              fb_check, adaptive_p2)


@_calc_cost_sgm_linear_op.register_fake
def _(I1, I2, pd0, nd, dMax, P1, P2, paths, subpixel, fb_check, adaptive_p2=0):
    return _matcher_outputs(I1, fb_check)


def _stereo_outputs(left, fb_check, ranged, minC2=None):
    """(disp, minC[, minC2], conf, disp2, status); disp / disp2 int32 true disparities for the entries that take d_min, else uint32"""
    disp, minC, conf, disp2, status = _matcher_outputs(left, fb_check, torch.int32 if ranged else torch.uint32)
    return (disp, minC) + _minC2_output(minC, minC2) + (conf, disp2, status)


def _stereo_run(fn, left, right, dMax, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2, *, d_min=None, minC2=None):
    """d_min: None for the entry without that argument (fsgm_stereo_sgm_device_opts)"""
    N, H, W, dev = _frames(left)
    left, right = _ready(left), _ready(right)
    disp, minC, *slot, conf, disp2, status = _stereo_outputs(left, fb_check, d_min is not None, minC2)
    prm = _stereo_params(paths, subpixel, direction, fb_check, dev.index)
    opt = _lib.options(adaptive_p2)
    _call(dev, fn, N, _p(left), _p(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
          *(() if d_min is None else (int(d_min),)), _p(disp), _p(minC), *_minC2_arg(slot, minC2), _p(conf) if fb_check else None,
          _p(disp2) if fb_check else None, _stream(dev), _p(status))
    return (disp, minC, *slot, conf, disp2, status)


@torch.library.custom_op("fsgm::stereo_sgm", mutates_args=())
def _stereo_sgm_op(left: torch.Tensor, right: torch.Tensor, dMax: int, P1: int, P2: int, paths: int, subpixel: int, direction: int,
                   fb_check: int, adaptive_p2: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _stereo_run(_L.fsgm_stereo_sgm_device_opts, left, right, dMax, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2)


@_stereo_sgm_op.register_fake
def _(left, right, dMax, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2=0):
    return _stereo_outputs(left, fb_check, False)


@torch.library.custom_op("fsgm::stereo_sgm_range", mutates_args=())
def _stereo_sgm_range_op(left: torch.Tensor, right: torch.Tensor, dMax: int, d_min: int, P1: int, P2: int, paths: int, subpixel: int,
                         direction: int, fb_check: int,
                         adaptive_p2: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _stereo_run(_L.fsgm_stereo_sgm_device_range, left, right, dMax, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2,
                       d_min=d_min)


@_stereo_sgm_range_op.register_fake
def _(left, right, dMax, d_min, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2=0):
    return _stereo_outputs(left, fb_check, True)


@torch.library.custom_op("fsgm::stereo_sgm_ru", mutates_args=())
def _stereo_sgm_ru_op(left: torch.Tensor, right: torch.Tensor, dMax: int, d_min: int, P1: int, P2: int, paths: int, subpixel: int,
                      direction: int, fb_check: int, adaptive_p2: int = 0
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::stereo_sgm_range with the runner-up cost minC2 after minC (fsgm_stereo_sgm_device_ru)"""
    return _stereo_run(_L.fsgm_stereo_sgm_device_ru, left, right, dMax, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2,
                       d_min=d_min, minC2=True)


@_stereo_sgm_ru_op.register_fake
def _(left, right, dMax, d_min, P1, P2, paths, subpixel, direction, fb_check, adaptive_p2=0):
    return _stereo_outputs(left, fb_check, True, True)


def _sgm_out_shape(C_, layout):
    if layout not in (0, 1):
        raise ValueError(f"layout must be 0 (hwd) or 1 (dhw), got {layout}")
    N, a, b, c = C_.shape
    return (N, a, b, c) if layout == 0 else (N, b, c, a)


def _sgm_outputs(C_, layout, return_sum, minC2=None):
    """(bestD, minC[, minC2], S, status); S is empty unless return_sum"""
    N, H, W, D = _sgm_out_shape(C_, layout)
    dev = C_.device
    minC = _u32((N, H, W), dev)
    return (_u32((N, H, W), dev), minC) + _minC2_output(minC, minC2) + (_u32((N, H, W, D) if return_sum else (0,), dev), _status(dev))


def _sgm_run(fn, C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum, minC2=None):
    N, H, W, D = _sgm_out_shape(C_, layout)
    dev = C_.device
    C_ = C_.contiguous()                                  # (any byte offset will do: the ingest kernel assumes no alignment)
    guide = guide.contiguous() if adaptive_p2 else None
    bestD, minC, *slot, S, status = _sgm_outputs(C_, layout, return_sum, minC2)
    prm = _sgm_params(_L, paths=paths, subpixel=subpixel, device=dev.index, agg_mode=agg_mode, layout="dhw" if layout else "hwd",
                      cost_bound=cost_bound, adaptive_p2=adaptive_p2)
    _call(dev, fn, N, _p(C_), W, H, D, int(P1), int(P2), C.byref(prm), _p(guide), _p(bestD), _p(minC), *_minC2_arg(slot, minC2),
          _p(S) if return_sum else None, _stream(dev), _p(status))
    return (bestD, minC, *slot, S, status)


@torch.library.custom_op("fsgm::sgm", mutates_args=())
def _sgm_op(C_: torch.Tensor, guide: torch.Tensor, P1: int, P2: int, paths: int, layout: int, cost_bound: int, agg_mode: int,
            adaptive_p2: int, subpixel: int, return_sum: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """C_ (N, H, W, D) for layout 0 or (N, D, H, W) for layout 1; guide (N, H, W), read with adaptive_p2 only."""
    return _sgm_run(_L.fsgm_sgm_device, C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum)


@_sgm_op.register_fake
def _(C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum):
    return _sgm_outputs(C_, layout, return_sum)


@torch.library.custom_op("fsgm::sgm_exact", mutates_args=())
def _sgm_exact_op(C_: torch.Tensor, guide: torch.Tensor, P1: int, P2: int, paths: int, layout: int, cost_bound: int, agg_mode: int,
                  adaptive_p2: int, subpixel: int, return_sum: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm with exact path arithmetic (fsgm_sgm_device_exact): P1, P2 in 0..255, the line kernels at every batch size"""
    return _sgm_run(_L.fsgm_sgm_device_exact, C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum)


@_sgm_exact_op.register_fake
def _(C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum):
    return _sgm_outputs(C_, layout, return_sum)


@torch.library.custom_op("fsgm::sgm_ru", mutates_args=())
def _sgm_ru_op(C_: torch.Tensor, guide: torch.Tensor, P1: int, P2: int, paths: int, layout: int, cost_bound: int, agg_mode: int,
               adaptive_p2: int, subpixel: int, return_sum: int
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm with the runner-up cost minC2 after minC (fsgm_sgm_device_ru): (bestD, minC, minC2, S, status)"""
    return _sgm_run(_L.fsgm_sgm_device_ru, C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum, True)


@_sgm_ru_op.register_fake
def _(C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum):
    return _sgm_outputs(C_, layout, return_sum, True)


def _sgm2d_out_shape(C_, layout, half_x, half_y):
    if layout not in (0, 1, 2):
        raise ValueError(f"layout must be 0 (hwd), 1 (dhw) or 2 (dhw_yx), got {layout}")
    n, H, W, D = _sgm2d_shape(tuple(C_.shape), "hwd" if layout == 0 else "dhw", half_x, half_y)
    if n is None:
        raise TypeError(f"fsgm::sgm2d takes batched costs (N, ...), got {tuple(C_.shape)}")
    return n, H, W, D


def _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum, minC2=None):
    """(bestD, minC[, minC2], mvSub, flow, S, status); flow / S are empty unless asked for"""
    N, H, W, D = _sgm2d_out_shape(C_, layout, half_x, half_y)
    dev = C_.device
    minC = _u32((N, H, W), dev)
    return ((_u32((N, H, W), dev), minC) + _minC2_output(minC, minC2)
            + (_f64((N, 2, H, W), dev), _f64((N, 2, H, W) if return_flow else (0,), dev), _u32((N, H, W, D) if return_sum else (0,), dev),
               _status(dev)))


_LAYOUT2D_NAMES = {code: name for name, code in _LAYOUTS2D.items()}


def _sgm2d_run(fn, who, C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel,
               return_flow, return_sum, minC2=None):
    """who: the op's name, for the one message that carries it"""
    N, H, W, D = _sgm2d_out_shape(C_, layout, half_x, half_y)
    dev = C_.device
    if not C_.is_contiguous():                            # (any byte offset will do: the ingest kernels assume no alignment)
        raise TypeError(f"{who} reads the costs where they lie: pass a contiguous tensor")
    have_hints = hints.numel() != 0
    hints = _ready(hints) if have_hints else None
    mvH, mvW = (hints.shape[-2], hints.shape[-1]) if have_hints else (0, 0)
    guide = guide.contiguous() if adaptive_p2 else None
    bestD, minC, *slot, mvSub, flow, S, status = _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum, minC2)
    prm = _sgm2d_params(_L, diagonal=diagonal, total_pass=total_pass, adaptive_p2=adaptive_p2, subpixel=subpixel, device=dev.index,
                        layout=_LAYOUT2D_NAMES[layout], cost_bound=cost_bound)
    _call(dev, fn, N, _p(C_), W, H, int(half_x), int(half_y), int(P1), int(P2), C.byref(prm), _p(hints), int(mvW), int(mvH), _p(guide),
          _p(bestD), _p(minC), *_minC2_arg(slot, minC2), _p(mvSub), _p(flow) if return_flow else None, _p(S) if return_sum else None,
          _stream(dev), _p(status))
    return (bestD, minC, *slot, mvSub, flow, S, status)


@torch.library.custom_op("fsgm::sgm2d", mutates_args=())
def _sgm2d_op(C_: torch.Tensor, hints: torch.Tensor, guide: torch.Tensor, half_x: int, half_y: int, P1: int, P2: int, layout: int,
              cost_bound: int, diagonal: int, total_pass: int, adaptive_p2: int, subpixel: int, return_flow: int,
              return_sum: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """C_ (N, H, W, D) for layout 0, (N, D, H, W) for 1 (channel sx*Sy + sy) and 2 (channel sy*Sx + sx); hints (N, 2, mvH, mvW)
    float64 or empty (zero hints); guide (N, H, W), read with adaptive_p2 only.  flow / S are empty unless asked for."""
    return _sgm2d_run(_L.fsgm_sgm2d_device, "fsgm::sgm2d", C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass,
                      adaptive_p2, subpixel, return_flow, return_sum)


@_sgm2d_op.register_fake
def _(C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel, return_flow, return_sum):
    return _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum)


@torch.library.custom_op("fsgm::sgm2d_ru", mutates_args=())
def _sgm2d_ru_op(C_: torch.Tensor, hints: torch.Tensor, guide: torch.Tensor, half_x: int, half_y: int, P1: int, P2: int, layout: int,
                 cost_bound: int, diagonal: int, total_pass: int, adaptive_p2: int, subpixel: int, return_flow: int, return_sum: int
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm2d with the runner-up cost minC2 after minC (fsgm_sgm2d_device_ru): (bestD, minC, minC2, mvSub, flow, S, status)"""
    return _sgm2d_run(_L.fsgm_sgm2d_device_ru, "fsgm::sgm2d_ru", C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass,
                      adaptive_p2, subpixel, return_flow, return_sum, True)


@_sgm2d_ru_op.register_fake
def _(C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel, return_flow, return_sum):
    return _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum, True)


@torch.library.custom_op("fsgm::sgm2d_exact", mutates_args=())
def _sgm2d_exact_op(C_: torch.Tensor, hints: torch.Tensor, guide: torch.Tensor, half_x: int, half_y: int, P1: int, P2: int, layout: int,
                    cost_bound: int, diagonal: int, total_pass: int, adaptive_p2: int, subpixel: int, return_flow: int, return_sum: int,
                    runner_up: bool
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm2d_ru with exact path arithmetic (fsgm_sgm2d_device_exact): P1, P2 in 0..255; minC2 is empty unless runner_up"""
    return _sgm2d_run(_L.fsgm_sgm2d_device_exact, "fsgm::sgm2d_exact", C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal,
                      total_pass, adaptive_p2, subpixel, return_flow, return_sum, bool(runner_up))


@_sgm2d_exact_op.register_fake
def _(C_, hints, guide, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel, return_flow, return_sum,
      runner_up):
    return _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum, bool(runner_up))


# Float cost volumes (include/fsgm.h, "Float cost volumes"): one op per family in a namespace of their own, fsgm_float::sgm and
# fsgm_float::sgm2d, each covering what the three u8 ops of its family cover -- runner_up and exact are flags, minC2 is the
# empty placeholder without runner_up.  The bodies are the u8 families': only the C entry, which quantises on the way in, differs.
_FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _float_entry(name, C_, scale, offset, exact):
    """The float entry `name` of the library as a callable with the argument list of its family's u8 _ru entry: the cost format
    of C_ goes in behind the volume, the exact switch in front of the stream.  The entry is looked up when the op runs."""
    if C_.dtype not in _FLOAT_DTYPES:
        raise TypeError(f"a float cost volume must be float32, float16 or bfloat16 (got {C_.dtype})")
    fmt = _cost_format(C_.dtype, scale, offset)

    def call(N, Cp, *rest):
        *mid, stream, status = rest
        return getattr(_L, name)(N, Cp, C.byref(fmt), *mid, int(bool(exact)), stream, status)
    return call


@torch.library.custom_op("fsgm_float::sgm", mutates_args=())
def _sgm_float_op(C_: torch.Tensor, guide: torch.Tensor, scale: float, offset: float, P1: int, P2: int, paths: int, layout: int,
                  cost_bound: int, agg_mode: int, adaptive_p2: int, subpixel: int, return_sum: int, runner_up: bool, exact: bool
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm / sgm_ru / sgm_exact on a float32 / float16 / bfloat16 volume (fsgm_sgm_float_dptr): (bestD, minC, minC2, S, status)"""
    return _sgm_run(_float_entry("fsgm_sgm_float_dptr", C_, scale, offset, exact), C_, guide, P1, P2, paths, layout, cost_bound, agg_mode,
                    adaptive_p2, subpixel, return_sum, bool(runner_up))


@_sgm_float_op.register_fake
def _(C_, guide, scale, offset, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum, runner_up, exact):
    return _sgm_outputs(C_, layout, return_sum, bool(runner_up))


@torch.library.custom_op("fsgm_float::sgm2d", mutates_args=())
def _sgm2d_float_op(C_: torch.Tensor, hints: torch.Tensor, guide: torch.Tensor, scale: float, offset: float, half_x: int, half_y: int,
                    P1: int, P2: int, layout: int, cost_bound: int, diagonal: int, total_pass: int, adaptive_p2: int, subpixel: int,
                    return_flow: int, return_sum: int, runner_up: bool, exact: bool
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm2d / sgm2d_ru / sgm2d_exact on a float volume (fsgm_sgm2d_float_dptr): (bestD, minC, minC2, mvSub, flow, S, status)"""
    return _sgm2d_run(_float_entry("fsgm_sgm2d_float_dptr", C_, scale, offset, exact), "fsgm_float::sgm2d", C_, hints, guide, half_x, half_y,
                      P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel, return_flow, return_sum, bool(runner_up))


@_sgm2d_float_op.register_fake
def _(C_, hints, guide, scale, offset, half_x, half_y, P1, P2, layout, cost_bound, diagonal, total_pass, adaptive_p2, subpixel, return_flow,
      return_sum, runner_up, exact):
    return _sgm2d_outputs(C_, layout, half_x, half_y, return_flow, return_sum, bool(runner_up))


# ---- the second view from the same aggregated volume (include/fsgm.h, "Second view"): a namespace of its own, fsgm_view2::, one op
# a family: minC2 is wanted or not (runner_up), exact a flag, as in fsgm_float:: ----
def _view2_sgm_outputs(C_, layout, return_sum, runner_up):
    """(bestD, minC, minC2, S, disp2, minC_v2, conf, status): fsgm::sgm_ru's with the second view's three maps before the status"""
    bestD, minC, minC2, S, status = _sgm_outputs(C_, layout, return_sum, bool(runner_up))
    return (bestD, minC, minC2, S, torch.empty_like(minC), torch.empty_like(minC), torch.empty(minC.shape, dtype=torch.uint8, device=minC.device),
            status)


@torch.library.custom_op("fsgm_view2::sgm", mutates_args=())
def _sgm_view2_op(C_: torch.Tensor, guide: torch.Tensor, P1: int, P2: int, paths: int, layout: int, cost_bound: int, agg_mode: int,
                  adaptive_p2: int, subpixel: int, return_sum: int, runner_up: bool, exact: bool, direction: int, d_min: int, max_diff: int
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::sgm / _ru / _exact with disp2, minC_v2 uint32 and conf uint8 (N, H, W) before the status (fsgm_sgm_view2_dptr)"""
    N, H, W, D = _sgm_out_shape(C_, layout)
    dev = C_.device
    C_ = C_.contiguous()
    guide = guide.contiguous() if adaptive_p2 else None
    bestD, minC, minC2, S, disp2, minC_v2, conf, status = _view2_sgm_outputs(C_, layout, return_sum, runner_up)
    prm = _sgm_params(_L, paths=paths, subpixel=subpixel, device=dev.index, agg_mode=agg_mode, layout="dhw" if layout else "hwd",
                      cost_bound=cost_bound, adaptive_p2=adaptive_p2)
    v2 = _view2_params(_L, direction, d_min, max_diff)
    _call(dev, _L.fsgm_sgm_view2_dptr, N, _p(C_), W, H, D, int(P1), int(P2), C.byref(prm), C.byref(v2), _p(guide), _p(bestD), _p(minC),
          _p(minC2) if runner_up else None, _p(S) if return_sum else None, int(bool(exact)), _p(disp2), _p(minC_v2), _p(conf), _stream(dev),
          _p(status))
    return bestD, minC, minC2, S, disp2, minC_v2, conf, status


@_sgm_view2_op.register_fake
def _(C_, guide, P1, P2, paths, layout, cost_bound, agg_mode, adaptive_p2, subpixel, return_sum, runner_up, exact, direction, d_min, max_diff):
    return _view2_sgm_outputs(C_, layout, return_sum, runner_up)


def _view2_stereo_outputs(left, runner_up):
    """(disp int32, minC, minC2, disp2 int32, minC_v2, conf, status)"""
    N, H, W, dev = _frames(left)
    minC = _u32((N, H, W), dev)
    i32 = lambda: torch.empty((N, H, W), dtype=torch.int32, device=dev)
    return (i32(), minC) + _minC2_output(minC, bool(runner_up)) + (i32(), _u32((N, H, W), dev),
                                                                   torch.empty((N, H, W), dtype=torch.uint8, device=dev), _status(dev))


@torch.library.custom_op("fsgm_view2::stereo_sgm", mutates_args=())
def _stereo_view2_op(left: torch.Tensor, right: torch.Tensor, dMax: int, d_min: int, P1: int, P2: int, paths: int, subpixel: int,
                     direction: int, adaptive_p2: int, runner_up: bool, max_diff: int
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::stereo_sgm_ru without fb_check, minC2 wanted or not, with disp2 int32, minC_v2 and conf (fsgm_stereo_sgm_view2_dptr)"""
    N, H, W, dev = _frames(left)
    left, right = _ready(left), _ready(right)
    disp, minC, minC2, disp2, minC_v2, conf, status = _view2_stereo_outputs(left, runner_up)
    prm = _stereo_params(paths, subpixel, direction, 0, dev.index)
    opt = _lib.options(adaptive_p2)
    _call(dev, _L.fsgm_stereo_sgm_view2_dptr, N, _p(left), _p(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt), int(d_min),
          int(max_diff), _p(disp), _p(minC), _p(minC2) if runner_up else None, _p(disp2), _p(minC_v2), _p(conf), _stream(dev), _p(status))
    return disp, minC, minC2, disp2, minC_v2, conf, status


@_stereo_view2_op.register_fake
def _(left, right, dMax, d_min, P1, P2, paths, subpixel, direction, adaptive_p2, runner_up, max_diff):
    return _view2_stereo_outputs(left, runner_up)


def _view2_check_outputs(disp):
    return torch.empty(disp.shape, dtype=torch.uint8, device=disp.device), _status(disp.device)


@torch.library.custom_op("fsgm_view2::check", mutates_args=())
def _view2_check_op(disp: torch.Tensor, disp2: torch.Tensor, direction: int, max_diff: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the left-right check alone on int32 true-disparity maps (N, H, W) (fsgm_view2_check_dptr)"""
    N, H, W, dev = _frames(disp)
    disp, disp2 = _ready(disp), _ready(disp2)
    conf, status = _view2_check_outputs(disp)
    _call(dev, _L.fsgm_view2_check_dptr, N, _p(disp), _p(disp2), W, H, int(direction), int(max_diff), _p(conf), dev.index, _stream(dev),
          _p(status))
    return conf, status


@_view2_check_op.register_fake
def _(disp, disp2, direction, max_diff):
    return _view2_check_outputs(disp)


def _epipolar_sgm_of_outputs(I0):
    N, H, W, dev = _frames(I0)
    return _f64((N, 3, H, W), dev), _u32((N, H, W), dev), _status(dev)


def _epipolar_flow_pp_outputs(I0):
    N, H, W, dev = _frames(I0)
    return _f64((N, 3, H, W), dev), _f64((N, 3, H, W), dev), _f64((N, H, W), dev), _u32((N, H, W), dev), _status(dev)


def _epipolar_run(fn, outputs, vz_to_disp, I0, I1, geometry, dMax, vMax, paths):
    """The epipolar drivers: `outputs` (I0) are the maps the entry writes, in its argument order, and the status"""
    N, H, W, dev = _frames(I0)
    ch = 1 if I0.dim() == 3 else 3
    g = _geometries(geometry, N)
    I0, I1 = _ready(I0), _ready(I1)
    *maps, status = outputs(I0)
    prm = _epi_params(paths, 1, vz_to_disp, dev.index, 0)
    _call(dev, fn, N, _p(I0), _p(I1), W, H, ch, g, int(dMax), float(vMax), C.byref(prm), *(_p(m) for m in maps), _stream(dev), _p(status))
    return (*maps, status)


@torch.library.custom_op("fsgm::epipolar_sgm_of", mutates_args=())
def _epipolar_sgm_of_op(I0: torch.Tensor, I1: torch.Tensor, geometry: List[float], dMax: int, vMax: float,
                        paths: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _epipolar_run(_L.fsgm_epipolar_sgm_of_device, _epipolar_sgm_of_outputs, 1, I0, I1, geometry, dMax, vMax, paths)


@_epipolar_sgm_of_op.register_fake
def _(I0, I1, geometry, dMax, vMax, paths):
    return _epipolar_sgm_of_outputs(I0)


@torch.library.custom_op("fsgm::epipolar_flow_pp", mutates_args=())
def _epipolar_flow_pp_op(I0: torch.Tensor, I1: torch.Tensor, geometry: List[float], dMax: int, vMax: float,
                         paths: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _epipolar_run(_L.fsgm_epipolar_flow_pp_device, _epipolar_flow_pp_outputs, 0, I0, I1, geometry, dMax, vMax, paths)


@_epipolar_flow_pp_op.register_fake
def _(I0, I1, geometry, dMax, vMax, paths):
    return _epipolar_flow_pp_outputs(I0)


def _epi_postprocess_outputs(D1):
    N, H, W, dev = _frames(D1)
    return _f64((N, H, W), dev), _f64((N, H, W), dev), _f64((N, H, W), dev), _status(dev)


@torch.library.custom_op("fsgm::epi_postprocess", mutates_args=())
def _epi_postprocess_op(D1: torch.Tensor, Pd0: torch.Tensor, nd: torch.Tensor, O: torch.Tensor, vMax: float, n: float,
                        dMax: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    N, H, W, dev = _frames(D1)
    D1, Pd0, nd, O = (_ready(t) for t in (D1, Pd0, nd, O))
    f1, f2, disp, status = _epi_postprocess_outputs(D1)
    _call(dev, _L.fsgm_epi_postprocess_device, N, _p(D1), W, H, _p(Pd0), _p(nd), _p(O), float(vMax), float(n), float(dMax),
          _p(f1), _p(f2), _p(disp), dev.index, _stream(dev), _p(status))
    return f1, f2, disp, status


@_epi_postprocess_op.register_fake
def _(D1, Pd0, nd, O, vMax, n, dMax):
    return _epi_postprocess_outputs(D1)


def _like(t):
    """the one output of the ops that map a flow to a flow of its shape"""
    return torch.empty_like(t, memory_format=torch.contiguous_format)


@torch.library.custom_op("fsgm::vmf", mutates_args=())
def _vmf_op(flow: torch.Tensor) -> torch.Tensor:
    N, ch, H, W = flow.shape
    dev = flow.device
    flow = _ready(flow)
    out = _like(flow)
    _call(dev, _L.fsgm_vmf_device, N, _p(flow), W, H, ch, _p(out), dev.index, _stream(dev))
    return out


@_vmf_op.register_fake
def _(flow):
    return _like(flow)


def _pyramid_outputs(I0, minC2=None):
    """(mv, minC[, minC2], status) of level 1"""
    N, H, W, dev = _frames(I0)
    minC = _u32((N, H, W), dev)
    return (_f64((N, 2, H, W), dev), minC) + _minC2_output(minC, minC2) + (_status(dev),)


def _pyramid_run(fn, prm, I0, I1, *, level_median=None, minC2=None):
    """level_median: None for an entry without that argument (the plain and the _ru ones)"""
    N, H, W, dev = _frames(I0)
    ch = 1 if I0.dim() == 3 else 3
    prm.device = dev.index
    I0, I1 = _ready(I0), _ready(I1)
    mv, minC, *slot, status = _pyramid_outputs(I0, minC2)
    _call(dev, fn, N, _p(I0), _p(I1), W, H, ch, C.byref(prm), *(() if level_median is None else (int(level_median),)), _p(mv), _p(minC),
          *_minC2_arg(slot, minC2), _stream(dev), _p(status))
    return (mv, minC, *slot, status)


def _pyramid_prm(default, fields, numPyd, params):
    prm = default()
    prm.numPyd = int(numPyd)
    for k, v in zip(fields, params, strict=True):
        setattr(prm, k, int(v))
    return prm


def _pyd_prm(numPyd, params):
    return _pyramid_prm(_L.fsgm_pyramid_params_default, PYRAMID_FIELDS, numPyd, params)


def _ng_prm(numPyd, params):
    return _pyramid_prm(_L.fsgm_ng_pyramid_params_default, NG_PYRAMID_FIELDS, numPyd, params)


@torch.library.custom_op("fsgm::pyramidal_sgm", mutates_args=())
def _pyramidal_sgm_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int,
                      params: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _pyramid_run(_L.fsgm_pyramidal_sgm_device, _pyd_prm(numPyd, params), I0, I1)


@_pyramidal_sgm_op.register_fake
def _(I0, I1, numPyd, params):
    return _pyramid_outputs(I0)


@torch.library.custom_op("fsgm::pyramidal_sgm_ng", mutates_args=())
def _pyramidal_sgm_ng_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int,
                         params: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _pyramid_run(_L.fsgm_pyramidal_sgm_ng_device, _ng_prm(numPyd, params), I0, I1)


@_pyramidal_sgm_ng_op.register_fake
def _(I0, I1, numPyd, params):
    return _pyramid_outputs(I0)


@torch.library.custom_op("fsgm::pyramidal_sgm_ru", mutates_args=())
def _pyramidal_sgm_ru_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int,
                         params: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _pyramid_run(_L.fsgm_pyramidal_sgm_device_ru, _pyd_prm(numPyd, params), I0, I1, minC2=True)


@_pyramidal_sgm_ru_op.register_fake
def _(I0, I1, numPyd, params):
    return _pyramid_outputs(I0, True)


@torch.library.custom_op("fsgm::pyramidal_sgm_ng_ru", mutates_args=())
def _pyramidal_sgm_ng_ru_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int,
                            params: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _pyramid_run(_L.fsgm_pyramidal_sgm_ng_device_ru, _ng_prm(numPyd, params), I0, I1, minC2=True)


@_pyramidal_sgm_ng_ru_op.register_fake
def _(I0, I1, numPyd, params):
    return _pyramid_outputs(I0, True)


@torch.library.custom_op("fsgm::pyramidal_sgm_lm", mutates_args=())
def _pyramidal_sgm_lm_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int, params: List[int], level_median: int,
                         runner_up: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::pyramidal_sgm_ru with the median between levels (fsgm_pyramidal_sgm_device_lm); minC2 is empty unless runner_up"""
    return _pyramid_run(_L.fsgm_pyramidal_sgm_device_lm, _pyd_prm(numPyd, params), I0, I1, level_median=level_median, minC2=bool(runner_up))


@_pyramidal_sgm_lm_op.register_fake
def _(I0, I1, numPyd, params, level_median, runner_up):
    return _pyramid_outputs(I0, bool(runner_up))


@torch.library.custom_op("fsgm::pyramidal_sgm_ng_lm", mutates_args=())
def _pyramidal_sgm_ng_lm_op(I0: torch.Tensor, I1: torch.Tensor, numPyd: int, params: List[int], level_median: int,
                            runner_up: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fsgm::pyramidal_sgm_ng_ru with the median between levels (fsgm_pyramidal_sgm_ng_device_lm); minC2 is empty unless runner_up"""
    return _pyramid_run(_L.fsgm_pyramidal_sgm_ng_device_lm, _ng_prm(numPyd, params), I0, I1, level_median=level_median, minC2=bool(runner_up))


@_pyramidal_sgm_ng_lm_op.register_fake
def _(I0, I1, numPyd, params, level_median, runner_up):
    return _pyramid_outputs(I0, bool(runner_up))


def _level_hints_output(flow):
    N, _, H, W = flow.shape
    return _f64((N, 2, 2 * H, 2 * W), flow.device)


@torch.library.custom_op("fsgm::flow_level_hints", mutates_args=())
def _flow_level_hints_op(flow: torch.Tensor, size: int) -> torch.Tensor:
    N, _, H, W = flow.shape
    dev = flow.device
    flow = _ready(flow)
    out = _level_hints_output(flow)
    _call(dev, _L.fsgm_flow_level_hints_device, N, _p(flow), W, H, int(size), _p(out), dev.index, _stream(dev))
    return out


@_flow_level_hints_op.register_fake
def _(flow, size):
    return _level_hints_output(flow)


def _pyramidal_flow_pp_outputs(I0, minC2=None):
    """(flow_pp, flow_checked, flow_fwd, flow_bwd, minC[, minC2], status)"""
    N, H, W, dev = _frames(I0)
    minC = _u32((N, H, W), dev)
    return ((_f64((N, 3, H, W), dev), _f64((N, 2, H, W), dev), _f64((N, 2, H, W), dev), _f64((N, 2, H, W), dev), minC)
            + _minC2_output(minC, minC2) + (_status(dev),))


def _flow_pp_prm(matcher, numPyd, params, chain, median, dev):
    prm = _L.fsgm_flow_pp_params_default(int(matcher))
    sub, fields = (prm.ng, NG_PYRAMID_FIELDS) if matcher == MATCHERS["ng"] else (prm.pyd, PYRAMID_FIELDS)
    sub.numPyd = int(numPyd)
    for k, v in zip(fields, params, strict=True):
        setattr(sub, k, int(v))
    for k, v in zip(FLOW_PP_FIELDS, chain, strict=True):
        setattr(prm, k, float(v))
    prm.median, prm.device = int(median), dev.index
    return prm


def _flow_pp_run(fn, I0, I1, matcher, numPyd, params, chain, median, *switches, minC2=None):
    """switches: the integers the entry takes after the parameter struct (uniqueness_ratio, then level_median)"""
    N, H, W, dev = _frames(I0)
    ch = 1 if I0.dim() == 3 else 3
    prm = _flow_pp_prm(matcher, numPyd, params, chain, median, dev)
    I0, I1 = _ready(I0), _ready(I1)
    pp, checked, fwd, bwd, minC, *slot, status = _pyramidal_flow_pp_outputs(I0, minC2)
    _call(dev, fn, N, _p(I0), _p(I1), W, H, ch, C.byref(prm), *(int(s) for s in switches), _p(pp), _p(checked), _p(fwd), _p(bwd), _p(minC),
          *_minC2_arg(slot, minC2), _stream(dev), _p(status))
    return (pp, checked, fwd, bwd, minC, *slot, status)


@torch.library.custom_op("fsgm::pyramidal_flow_pp", mutates_args=())
def _pyramidal_flow_pp_op(I0: torch.Tensor, I1: torch.Tensor, matcher: int, numPyd: int, params: List[int], chain: List[float],
                          median: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _flow_pp_run(_L.fsgm_pyramidal_flow_pp_device, I0, I1, matcher, numPyd, params, chain, median)


@_pyramidal_flow_pp_op.register_fake
def _(I0, I1, matcher, numPyd, params, chain, median):
    return _pyramidal_flow_pp_outputs(I0)


@torch.library.custom_op("fsgm::pyramidal_flow_pp_u", mutates_args=())
def _pyramidal_flow_pp_u_op(I0: torch.Tensor, I1: torch.Tensor, matcher: int, numPyd: int, params: List[int], chain: List[float],
                            median: int, uniqueness_ratio: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                                         torch.Tensor, torch.Tensor, torch.Tensor]:
    return _flow_pp_run(_L.fsgm_pyramidal_flow_pp_device_u, I0, I1, matcher, numPyd, params, chain, median, uniqueness_ratio, minC2=True)


@_pyramidal_flow_pp_u_op.register_fake
def _(I0, I1, matcher, numPyd, params, chain, median, uniqueness_ratio):
    return _pyramidal_flow_pp_outputs(I0, True)


@torch.library.custom_op("fsgm::pyramidal_flow_pp_lm", mutates_args=())
def _pyramidal_flow_pp_lm_op(I0: torch.Tensor, I1: torch.Tensor, matcher: int, numPyd: int, params: List[int], chain: List[float],
                             median: int, uniqueness_ratio: int, want_minC2: bool,
                             level_median: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                         torch.Tensor, torch.Tensor]:
    """fsgm::pyramidal_flow_pp_u with the median between levels (fsgm_pyramidal_flow_pp_device_lm); minC2 is empty unless
    want_minC2, which a non-zero uniqueness_ratio needs"""
    return _flow_pp_run(_L.fsgm_pyramidal_flow_pp_device_lm, I0, I1, matcher, numPyd, params, chain, median, uniqueness_ratio, level_median,
                        minC2=bool(want_minC2))


@_pyramidal_flow_pp_lm_op.register_fake
def _(I0, I1, matcher, numPyd, params, chain, median, uniqueness_ratio, want_minC2, level_median):
    return _pyramidal_flow_pp_outputs(I0, bool(want_minC2))


@torch.library.custom_op("fsgm::flow_fb_check", mutates_args=())
def _flow_fb_check_op(f: torch.Tensor, b: torch.Tensor, thr: float) -> torch.Tensor:
    N, _, H, W = f.shape
    dev = f.device
    f, b = _ready(f), _ready(b)
    out = _like(f)
    _call(dev, _L.fsgm_flow_fb_check_device, N, _p(f), _p(b), W, H, float(thr), _p(out), dev.index, _stream(dev))
    return out


@_flow_fb_check_op.register_fake
def _(f, b, thr):
    return _like(f)


def _stereo_sgm_pp_outputs(left):
    N, H, W, dev = _frames(left)
    return (_f64((N, H, W), dev), _f64((N, H, W), dev), torch.empty((N, H, W), dtype=torch.int32, device=dev), _u32((N, H, W), dev),
            _f64((N, H, W), dev), _status(dev))


@torch.library.custom_op("fsgm::stereo_sgm_pp", mutates_args=())
def _stereo_sgm_pp_op(left: torch.Tensor, right: torch.Tensor, dMax: int, d_min: int, P1: int, P2: int, paths: int, subpixel: int,
                      direction: int, adaptive_p2: int, chain: List[float],
                      in_fill: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    N, H, W, dev = _frames(left)
    left, right = _ready(left), _ready(right)
    disp_pp, checked, disp, minC, disp2, status = _stereo_sgm_pp_outputs(left)
    prm = _stereo_params(paths, subpixel, direction, 0, dev.index)
    opt = _lib.options(adaptive_p2)
    pp = _stereo_pp_params(_L, in_fill, dict(zip(STEREO_PP_FIELDS, chain, strict=True)))
    _call(dev, _L.fsgm_stereo_sgm_pp_device, N, _p(left), _p(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
          int(d_min), C.byref(pp), _p(disp_pp), _p(checked), _p(disp), _p(minC), _p(disp2), _stream(dev), _p(status))
    return disp_pp, checked, disp, minC, disp2, status


@_stereo_sgm_pp_op.register_fake
def _(left, right, dMax, d_min, P1, P2, paths, subpixel, direction, adaptive_p2, chain, in_fill):
    return _stereo_sgm_pp_outputs(left)


def _stereo_fb_check_outputs(D1, fused):
    N, H, W, dev = _frames(D1)
    return _f64((N, H, W), dev), _f64((N, H, W) if fused else (0,), dev), _status(dev)


@torch.library.custom_op("fsgm::stereo_fb_check", mutates_args=())
def _stereo_fb_check_op(D1: torch.Tensor, D2: torch.Tensor, fused: int, d_min: int, direction: int,
                        thr: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fused: D2 is not read, the second-view map is made from D1 and returned; else the check alone against D2."""
    N, H, W, dev = _frames(D1)
    D1 = _ready(D1)
    D2 = None if fused else _ready(D2)                   # (a local: a contiguous copy must outlive the call)
    out, second, status = _stereo_fb_check_outputs(D1, fused)
    _call(dev, _L.fsgm_stereo_fb_check_device, N, _p(D1), _p(D2), W, H, int(d_min), int(direction), float(thr),
          _p(out), _p(second) if fused else None, dev.index, _stream(dev), _p(status))
    return out, second, status


@_stereo_fb_check_op.register_fake
def _(D1, D2, fused, d_min, direction, thr):
    return _stereo_fb_check_outputs(D1, fused)


def _uniqueness_planes_check(map_, minC, minC2, planes):
    """the raw op's own shape check: the kernel indexes N * planes * H * W elements of map_ and N * H * W of the costs"""
    if planes not in (1, 2):
        raise ValueError(f"fsgm::uniqueness_filter_planes: planes must be 1 or 2 (got {planes})")
    if minC.dim() != 3 or tuple(minC2.shape) != tuple(minC.shape):
        raise TypeError(f"fsgm::uniqueness_filter_planes: minC and minC2 must be (N, H, W) of one shape (got {tuple(minC.shape)}, "
                        f"{tuple(minC2.shape)})")
    N, H, W = minC.shape
    want = (N, H, W) if planes == 1 else (N, 2, H, W)
    if tuple(map_.shape) != want:
        raise TypeError(f"fsgm::uniqueness_filter_planes: map_ must be {want} with planes {planes} (got {tuple(map_.shape)})")


def _uniqueness_filter_outputs(map_):
    return torch.empty_like(map_, memory_format=torch.contiguous_format), _status(map_.device)


@torch.library.custom_op("fsgm::uniqueness_filter", mutates_args=())
def _uniqueness_filter_op(map_: torch.Tensor, minC: torch.Tensor, minC2: torch.Tensor, ratio: int) -> Tuple[torch.Tensor, torch.Tensor]:
    N, H, W, dev = _frames(map_)
    map_, minC, minC2 = _ready(map_), _ready(minC), _ready(minC2)
    out, status = _uniqueness_filter_outputs(map_)
    _call(dev, _L.fsgm_uniqueness_filter_device, N, _p(map_), _p(minC), _p(minC2), W, H, int(ratio), _p(out), dev.index, _stream(dev),
          _p(status))
    return out, status


@_uniqueness_filter_op.register_fake
def _(map_, minC, minC2, ratio):
    return _uniqueness_filter_outputs(map_)


@torch.library.custom_op("fsgm::uniqueness_filter_planes", mutates_args=())
def _uniqueness_filter_planes_op(map_: torch.Tensor, minC: torch.Tensor, minC2: torch.Tensor, ratio: int,
                                 planes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """map_ (N, H, W) with planes 1, (N, 2, H, W) with planes 2; minC, minC2 (N, H, W)"""
    _uniqueness_planes_check(map_, minC, minC2, planes)
    N, H, W, dev = _frames(minC)
    map_, minC, minC2 = _ready(map_), _ready(minC), _ready(minC2)
    out, status = _uniqueness_filter_outputs(map_)
    _call(dev, _L.fsgm_uniqueness_filter_planes_device, N, _p(map_), _p(minC), _p(minC2), W, H, int(planes), int(ratio), _p(out), dev.index,
          _stream(dev), _p(status))
    return out, status


@_uniqueness_filter_planes_op.register_fake
def _(map_, minC, minC2, ratio, planes):
    _uniqueness_planes_check(map_, minC, minC2, planes)
    return _uniqueness_filter_outputs(map_)


# ---------------------------------------------------------------------------------------------
# wrappers: the argument order of the numpy API, one frame or a batch with a leading N
# ---------------------------------------------------------------------------------------------
def _tensors(named, device=None):
    """TypeError unless every value is a GPU tensor of the dtype asked for (a tuple: of one of them), all on one device; returns that device."""
    for name, (t, dtype) in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor (got {type(t).__name__})")
        if t.device.type != "cuda":
            raise TypeError(f"{name} is on {t.device}: pass tensors on the GPU (no silent transfer)")
        if isinstance(dtype, tuple):
            if t.dtype not in dtype:
                raise TypeError(f"{name} must be one of {', '.join(str(d) for d in dtype)} (got {t.dtype})")
        elif t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
        if device is None:
            device = t.device
        elif t.device != device:
            raise TypeError(f"{name} is on {t.device}, the other arguments on {device}")
    return device


def _shape(name, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise TypeError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")


def _finish(outs, status, batched, check, return_status, why="an aggregation hand-off gave up"):
    if check:
        torch.cuda.current_stream(status.device).synchronize()
        s = int(status.item())
        if s != 0:
            raise FsgmError(s, f"the device reported a failed run ({why}): results are invalid")
    outs = tuple(outs if batched else (o[0] for o in outs))
    return outs + (status,) if return_status else outs


def calc_cost_sgm(I1, I2, dMax, vMax, pixelPosD0, normlizeDirection, offsetFromPosD0, P1, P2, *, paths=4, subpixel=1,
                  vz_to_disp=1, fb_check=0, check=False, return_status=False, adaptive_p2=0):
    """[bestD, minC] = calc_cost_sgm(...) as fsgm_amd.calc_cost_sgm, on torch tensors on the GPU.  One frame: I1, I2 (H, W) uint8,
    pixelPosD0 / normlizeDirection (2, H, W) and offsetFromPosD0 (H, W) float64; a batch: the same with a leading N.
    Returns uint32 tensors of the same leading shape (and conf uint8 / bestD2 uint32 with fb_check=1; the status tensor last
    with return_status=True).  check=True synchronises the current stream and raises FsgmError on a non-zero status.
    adaptive_p2=1: the reference's edge-aware large penalty (calc_cost_sgm.cpp:68-72), as fsgm_amd.calc_cost_sgm."""
    _tensors({"I1": (I1, torch.uint8), "I2": (I2, torch.uint8), "pixelPosD0": (pixelPosD0, torch.float64),
                    "normlizeDirection": (normlizeDirection, torch.float64), "offsetFromPosD0": (offsetFromPosD0, torch.float64)})
    if I1.dim() not in (2, 3):
        raise TypeError(f"I1 must be (H, W) or (N, H, W) (got {tuple(I1.shape)})")
    batched = I1.dim() == 3
    lead = tuple(I1.shape[:-2])
    H, W = I1.shape[-2:]
    _shape("I2", I2, lead + (H, W))
    _shape("pixelPosD0", pixelPosD0, lead + (2, H, W))
    _shape("normlizeDirection", normlizeDirection, lead + (2, H, W))
    _shape("offsetFromPosD0", offsetFromPosD0, lead + (H, W))
    if not batched:
        I1, I2, pixelPosD0, normlizeDirection, offsetFromPosD0 = (t.unsqueeze(0) for t in (I1, I2, pixelPosD0, normlizeDirection, offsetFromPosD0))
    bestD, minC, conf, bestD2, status = torch.ops.fsgm.calc_cost_sgm(I1, I2, pixelPosD0, normlizeDirection, offsetFromPosD0, int(dMax),
                                                                      float(vMax), int(P1), int(P2), int(paths), int(subpixel),
                                                                      int(vz_to_disp), int(fb_check), int(adaptive_p2))
    outs = (bestD, minC, conf, bestD2) if fb_check else (bestD, minC)
    return _finish(outs, status, batched, check, return_status)


def calc_cost_sgm_linear(I1, I2, dMax, pixelPosD0, normlizeDirection, P1, P2, *, paths=4, subpixel=1, fb_check=0, check=False,
                         return_status=False, adaptive_p2=0):
    """[bestD, minC] as fsgm_amd.calc_cost_sgm_linear (the reference built without USE_VZIND), on torch tensors on the GPU.  One
    frame: I1, I2 (H, W) uint8, pixelPosD0 / normlizeDirection (2, H, W) float64; a batch: the same with a leading N.  Outputs,
    fb_check, check, return_status and adaptive_p2 as calc_cost_sgm."""
    _tensors({"I1": (I1, torch.uint8), "I2": (I2, torch.uint8), "pixelPosD0": (pixelPosD0, torch.float64),
              "normlizeDirection": (normlizeDirection, torch.float64)})
    if I1.dim() not in (2, 3):
        raise TypeError(f"I1 must be (H, W) or (N, H, W) (got {tuple(I1.shape)})")
    batched = I1.dim() == 3
    lead = tuple(I1.shape[:-2])
    H, W = I1.shape[-2:]
    _shape("I2", I2, lead + (H, W))
    _shape("pixelPosD0", pixelPosD0, lead + (2, H, W))
    _shape("normlizeDirection", normlizeDirection, lead + (2, H, W))
    if not batched:
        I1, I2, pixelPosD0, normlizeDirection = (t.unsqueeze(0) for t in (I1, I2, pixelPosD0, normlizeDirection))
    bestD, minC, conf, bestD2, status = torch.ops.fsgm.calc_cost_sgm_linear(I1, I2, pixelPosD0, normlizeDirection, int(dMax), int(P1),
                                                                             int(P2), int(paths), int(subpixel), int(fb_check),
                                                                             int(adaptive_p2))
    outs = (bestD, minC, conf, bestD2) if fb_check else (bestD, minC)
    return _finish(outs, status, batched, check, return_status)


def sgm(Cvol, P1=7, P2=100, *, layout="dhw", paths=4, cost_bound=255, agg_mode=0, adaptive_p2=0, guide=None, subpixel=1,
        return_sum=False, check=False, return_status=False, runner_up=False, arith="mod256", second_view=False, direction=-1, d_min=0,
        max_diff=256):
    """bestD, minC = sgm(C, P1, P2) as fsgm_amd.sgm_batch, on a cost volume that is already in HBM: C uint8 (D, H, W) or a batch
    (N, D, H, W) for layout "dhw" (a cost-volume network's output), (H, W, D) / (N, H, W, D) for "hwd".  The volume is read where
    it lies, every output stays in HBM, the work is queued on the current stream.  bestD, minC uint32 (.., H, W); return_sum
    adds S uint32 (.., H, W, D).  cost_bound: the caller's declaration that no cost is larger; the kernels are selected for it
    and every cost is saturated at it on the way in.  The status tensor (return_status=True) is FSGM_ERR_INVALID when a cost was
    above the bound (the outputs are then those of the saturated volume), FSGM_ERR_HIP when an aggregation hand-off gave up;
    check=True synchronises and raises on either.  adaptive_p2=1 needs guide, the first image, uint8 (.., H, W).  runner_up=True
    (fsgm::sgm_ru) returns minC2 uint32 after minC, as fsgm_amd.sgm_batch does.  arith="exact" (fsgm::sgm_exact): path costs that
    are never narrowed to a byte, as fsgm_amd.sgm_batch(arith="exact") -- P1, P2 in 0..255, the line kernels at every batch size;
    with runner_up=True it raises ValueError.  second_view=True (fsgm_view2::sgm) appends disp2, minC_v2 uint32 and conf uint8: the
    second view's disparity from the same aggregated volume and the left-right check, as fsgm_amd.sgm_batch(second_view=True) with
    its direction, d_min and max_diff."""
    return _sgm_call(Cvol, None, P1, P2, layout, paths, cost_bound, agg_mode, adaptive_p2, guide, subpixel, return_sum, check, return_status,
                     runner_up, arith, (int(direction), int(d_min), int(max_diff)) if second_view else None)


def sgm_float(Cvol, scale, offset=0.0, P1=7, P2=100, *, layout="dhw", paths=4, cost_bound=255, agg_mode=0, adaptive_p2=0, guide=None,
              subpixel=1, return_sum=False, check=False, return_status=False, runner_up=False, arith="mod256"):
    """sgm on a float cost volume (fsgm_float::sgm, fsgm_sgm_float_dptr): C float32, float16 or bfloat16 in the shapes sgm takes,
    e.g. a cost-volume network's (N, D, H, W) output.  Each voxel c is quantised in the kernel pass that brings the volume into
    the plan -- q = clamp(rint(float32(c) * scale + offset), 0, cost_bound): one float32 multiply, one float32 add, ties to even,
    scale and offset rounded to float32 first; a negative scale turns a similarity into a cost -- and the u8 path runs on the
    bytes: every output is, bit for bit, that of sgm on q with the same cost_bound.  A voxel that rounds below 0 or above
    cost_bound, or a NaN, sets the status to FSGM_ERR_INVALID (the outputs are those of the clamped volume); check=True raises on
    it.  The volume is read where it lies: a contiguous slice of a larger tensor will do.  Everything else as sgm."""
    return _sgm_call(Cvol, (float(scale), float(offset)), P1, P2, layout, paths, cost_bound, agg_mode, adaptive_p2, guide, subpixel,
                     return_sum, check, return_status, runner_up, arith)


def _sgm_call(Cvol, quant, P1, P2, layout, paths, cost_bound, agg_mode, adaptive_p2, guide, subpixel, return_sum, check, return_status,
              runner_up, arith, view2=None):
    """sgm (quant None: a uint8 volume; view2 = (direction, d_min, max_diff): through fsgm_view2::sgm) and sgm_float (quant = (scale, offset): a float volume, through fsgm_float::sgm)"""
    exact = _arith_exact(arith)
    if exact and runner_up:
        raise ValueError("arith='exact' has no runner-up cost: runner_up=True needs arith='mod256'")
    code = _layout_code(layout)
    named = {"C": (Cvol, torch.uint8 if quant is None else _FLOAT_DTYPES)}
    if guide is not None:
        named["guide"] = (guide, torch.uint8)
    _tensors(named)
    n, H, W, D = _sgm_shape(Cvol.shape, layout)
    batched = n is not None
    if int(adaptive_p2) not in (0, 1):
        raise ValueError(f"adaptive_p2 must be 0 or 1 (got {adaptive_p2!r})")
    if guide is not None:                                  # (adaptive_p2 without one: the library refuses, status 1)
        _shape("guide", guide, ((n,) if batched else ()) + (H, W))
    if not batched:
        Cvol = Cvol.unsqueeze(0)
        guide = None if guide is None else guide.unsqueeze(0)
    if guide is None or not adaptive_p2:
        guide = torch.empty((0,), dtype=torch.uint8, device=Cvol.device)
    args = (Cvol, guide, int(P1), int(P2), int(paths), code, int(cost_bound), int(agg_mode), int(adaptive_p2), int(subpixel),
            int(bool(return_sum)))
    extra = ()
    if view2 is not None:
        bestD, minC, minC2, S, *extra, status = torch.ops.fsgm_view2.sgm(*args, bool(runner_up), exact, *view2)
    elif quant is not None:
        bestD, minC, minC2, S, status = torch.ops.fsgm_float.sgm(*args[:2], *quant, *args[2:], bool(runner_up), exact)
    elif runner_up:
        bestD, minC, minC2, S, status = torch.ops.fsgm.sgm_ru(*args)
    elif exact:
        bestD, minC, S, status = torch.ops.fsgm.sgm_exact(*args)
    else:
        bestD, minC, S, status = torch.ops.fsgm.sgm(*args)
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + ((S,) if return_sum else ()) + tuple(extra)
    return _finish(outs, status, batched, check, return_status, "a cost above cost_bound, or an aggregation hand-off that gave up")


def sgm2d(costs, half_x, half_y, P1=6, P2=32, *, layout="dhw", hints=None, guide=None, cost_bound=255, diagonal=1, total_pass=2,
          adaptive_p2=0, subpixel=1, return_flow=False, return_sum=False, check=False, return_status=False, runner_up=False,
          arith="wrap"):
    """(bestD, minC[, minC2], mvSub[, flow][, S]) as fsgm_amd.sgm2d_batch, on cost volumes that are already in HBM: costs uint8 (D, H, W) or
    a batch (N, D, H, W) for layout "dhw" (channel sx*Sy + sy) and "dhw_yx" (channel sy*Sx + sx, a correlation layer's order),
    (H, W, D) / (N, H, W, D) for "hwd".  The tensor is read where it lies -- it must be contiguous, at any byte address -- every
    output stays in HBM, the work is queued on the current stream.  hints float64 (.., 2, mvH, mvW) or None (zeros), guide uint8
    (.., H, W) with adaptive_p2=1.  bestD, minC uint32 (.., H, W); mvSub and flow float64 (.., 2, H, W); S uint32 (.., H, W, D).
    cost_bound: the caller's declaration that no cost is larger; the aggregation is selected for it and every cost is saturated at
    it on the way in.  The status tensor (return_status=True) is FSGM_ERR_INVALID when a cost was above the bound (the outputs are
    then those of the saturated volume); check=True synchronises and raises on it.  runner_up=True (fsgm::sgm2d_ru) returns minC2
    uint32 (.., H, W) after minC, as fsgm_amd.sgm2d_batch does.  arith="exact" (fsgm::sgm2d_exact): path costs that are never
    narrowed to a byte, as fsgm_amd.sgm2d_batch(arith="exact") -- P1, P2 in 0..255, "generic/exact" at every window and bound, with or
    without runner_up."""
    return _sgm2d_call(costs, None, half_x, half_y, P1, P2, layout, hints, guide, cost_bound, diagonal, total_pass, adaptive_p2, subpixel,
                       return_flow, return_sum, check, return_status, runner_up, arith)


def sgm2d_float(costs, half_x, half_y, scale, offset=0.0, P1=6, P2=32, *, layout="dhw", hints=None, guide=None, cost_bound=255, diagonal=1,
                total_pass=2, adaptive_p2=0, subpixel=1, return_flow=False, return_sum=False, check=False, return_status=False,
                runner_up=False, arith="wrap"):
    """sgm2d on a float cost volume (fsgm_float::sgm2d, fsgm_sgm2d_float_dptr): costs float32, float16 or bfloat16 in the shapes
    sgm2d takes, e.g. a correlation layer's (N, 81, H, W) for a 9x9 window with layout "dhw_yx".  Each voxel c is quantised in the
    kernel pass that brings the volume into the plan -- q = clamp(rint(float32(c) * scale + offset), 0, cost_bound), as
    sgm_float; a negative scale turns a correlation into a cost -- and the u8 path runs on the bytes: every output is, bit for
    bit, that of sgm2d on q with the same cost_bound.  A voxel that rounds below 0 or above cost_bound, or a NaN, sets the status to
    FSGM_ERR_INVALID (the outputs are those of the clamped volume).  The tensor must be contiguous and may be a slice of a larger
    one.  Everything else as sgm2d."""
    return _sgm2d_call(costs, (float(scale), float(offset)), half_x, half_y, P1, P2, layout, hints, guide, cost_bound, diagonal, total_pass,
                       adaptive_p2, subpixel, return_flow, return_sum, check, return_status, runner_up, arith)


def _sgm2d_call(costs, quant, half_x, half_y, P1, P2, layout, hints, guide, cost_bound, diagonal, total_pass, adaptive_p2, subpixel,
                return_flow, return_sum, check, return_status, runner_up, arith):
    """sgm2d (quant None: a uint8 volume) and sgm2d_float (quant = (scale, offset): a float volume, through fsgm_float::sgm2d)"""
    exact = _arith2d_exact(arith)
    code = _layout2d_code(layout)
    named = {"costs": (costs, torch.uint8 if quant is None else _FLOAT_DTYPES)}
    if hints is not None:
        named["hints"] = (hints, torch.float64)
    if guide is not None:
        named["guide"] = (guide, torch.uint8)
    _tensors(named)
    n, H, W, D = _sgm2d_shape(tuple(costs.shape), layout, half_x, half_y)
    batched = n is not None
    lead = (n,) if batched else ()
    if not costs.is_contiguous():
        raise TypeError("costs must be contiguous: the volume is read where it lies (no silent copy)")
    if int(adaptive_p2) not in (0, 1):
        raise ValueError(f"adaptive_p2 must be 0 or 1 (got {adaptive_p2!r})")
    if hints is not None:
        if hints.dim() != len(lead) + 3 or tuple(hints.shape[:-2]) != lead + (2,):
            raise TypeError(f"hints must have shape {lead + (2, 'mvH', 'mvW')} (got {tuple(hints.shape)})")
        if hints.shape[-2] < H or hints.shape[-1] < W:
            raise ValueError(f"hints ({hints.shape[-2]} x {hints.shape[-1]}) must be at least as large as the image ({H} x {W})")
    if guide is not None:                                  # (adaptive_p2 without one: the library refuses, status 1)
        _shape("guide", guide, lead + (H, W))
    if not batched:
        costs = costs.unsqueeze(0)
        hints = None if hints is None else hints.unsqueeze(0)
        guide = None if guide is None else guide.unsqueeze(0)
    dev = costs.device
    if hints is None:
        hints = torch.empty((0,), dtype=torch.float64, device=dev)
    if guide is None or not adaptive_p2:
        guide = torch.empty((0,), dtype=torch.uint8, device=dev)
    args = (costs, hints, guide, int(half_x), int(half_y), int(P1), int(P2), code, int(cost_bound), int(diagonal), int(total_pass),
            int(adaptive_p2), int(subpixel), int(bool(return_flow)), int(bool(return_sum)))
    if quant is not None:
        bestD, minC, minC2, mvSub, flow, S, status = torch.ops.fsgm_float.sgm2d(*args[:3], *quant, *args[3:], bool(runner_up), exact)
    elif exact:
        bestD, minC, minC2, mvSub, flow, S, status = torch.ops.fsgm.sgm2d_exact(*args, bool(runner_up))
    elif runner_up:
        bestD, minC, minC2, mvSub, flow, S, status = torch.ops.fsgm.sgm2d_ru(*args)
    else:
        bestD, minC, mvSub, flow, S, status = torch.ops.fsgm.sgm2d(*args)
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + (mvSub,) + ((flow,) if return_flow else ()) + ((S,) if return_sum else ())
    return _finish(outs, status, batched, check, return_status, "a cost above cost_bound")


def _ingest(plan, t, name, layout, code, must_be_contiguous, fn, cost_bound, check, return_status, quant=None):
    """`plan.batch` cost volumes from the uint8 tensor `t` (called `name` in messages) through a plan's ingest entry `fn`; `code` is
    the entry's number for `layout`.  A tensor that is not contiguous is refused with must_be_contiguous, else copied.
    quant = (scale, offset): `t` is a float volume and `fn` the entry's float form, which takes the cost format behind the volume."""
    dev = _tensors({name: (t, torch.uint8 if quant is None else _FLOAT_DTYPES)})
    if dev.index != plan.device:
        raise TypeError(f"the tensor is on {dev}, the plan on device {plan.device}")
    _shape(name, t, (plan.batch, plan.H, plan.W, plan.D) if layout == "hwd" else (plan.batch, plan.D, plan.H, plan.W))
    if must_be_contiguous and not t.is_contiguous():
        raise TypeError(f"{name} must be contiguous: the volume is read where it lies (no silent copy)")
    t = t.contiguous()
    status = _status(dev)
    fmt = () if quant is None else (C.byref(_cost_format(t.dtype, *quant)),)
    _call(dev, fn, plan._h, plan.batch, _p(t), *fmt, code, int(cost_bound), _stream(dev), _p(status))
    res = _finish((), status, True, check, return_status, "a cost above cost_bound")
    return res[0] if return_status else None


def ingest_cost(plan, Cvol, *, layout="dhw", cost_bound=255, check=False, return_status=False):
    """All `plan.batch` cost volumes of an EpiPlan from a uint8 tensor on the plan's GPU (fsgm_epi_plan_ingest_cost_device): (N, D, H, W)
    for layout "dhw", (N, H, W, D) for "hwd", saturated at cost_bound, which the plan then selects its kernels by.  What
    EpiPlan.upload_cost does from the host, frame by frame.  Returns the status tensor with return_status=True, else None."""
    return _ingest(plan, Cvol, "C", layout, _layout_code(layout), False, _L.fsgm_epi_plan_ingest_cost_device, cost_bound, check, return_status)


def ingest_cost2d(plan, costs, *, layout="dhw", cost_bound=255, check=False, return_status=False):
    """All `plan.batch` cost volumes of a PydPlan from a uint8 tensor on the plan's GPU (fsgm_pyd_plan_ingest_cost_device):
    (N, D, H, W) for layout "dhw" / "dhw_yx", (N, H, W, D) for "hwd", saturated at cost_bound, which the plan then selects its
    aggregation by.  What PydPlan.upload_cost does from the host, frame by frame.  Returns the status tensor with
    return_status=True, else None."""
    return _ingest(plan, costs, "costs", layout, _layout2d_code(layout), True, _L.fsgm_pyd_plan_ingest_cost_device, cost_bound, check,
                   return_status)


def ingest_cost_float(plan, Cvol, scale, offset=0.0, *, layout="dhw", cost_bound=255, check=False, return_status=False):
    """ingest_cost for a float32 / float16 / bfloat16 tensor (fsgm_epi_plan_ingest_float_dptr): every voxel quantised to
    clamp(rint(float32(c) * scale + offset), 0, cost_bound) on the way into the plan, as sgm_float does; the status is
    FSGM_ERR_INVALID when a voxel rounded outside 0..cost_bound or was a NaN."""
    return _ingest(plan, Cvol, "C", layout, _layout_code(layout), False, _L.fsgm_epi_plan_ingest_float_dptr, cost_bound, check, return_status,
                   (float(scale), float(offset)))


def ingest_cost2d_float(plan, costs, scale, offset=0.0, *, layout="dhw", cost_bound=255, check=False, return_status=False):
    """ingest_cost2d for a float32 / float16 / bfloat16 tensor (fsgm_pyd_plan_ingest_float_dptr), quantised as sgm2d_float does."""
    return _ingest(plan, costs, "costs", layout, _layout2d_code(layout), True, _L.fsgm_pyd_plan_ingest_float_dptr, cost_bound, check,
                   return_status, (float(scale), float(offset)))


def _stereo_inputs(left, right, dMax, paths, subpixel, direction, fb_check, adaptive_p2):
    """The checks the rectified-stereo wrappers share, before anything is queued; returns (left, right with a leading N, batched)."""
    _tensors({"left": (left, torch.uint8), "right": (right, torch.uint8)})
    if left.dim() not in (2, 3):
        raise TypeError(f"left must be (H, W) or (N, H, W) (got {tuple(left.shape)})")
    _shape("right", right, left.shape)
    if int(dMax) < 1:
        raise ValueError(f"dMax must be >= 1 (got {dMax!r})")
    _stereo_params(paths, subpixel, direction, fb_check, 0)                 # the value checks
    if int(adaptive_p2) not in (0, 1):
        raise ValueError(f"adaptive_p2 must be 0 or 1 (got {adaptive_p2!r})")
    if left.dim() == 3:
        return left, right, True
    return left.unsqueeze(0), right.unsqueeze(0), False


def stereo_sgm(left, right, dMax, P1=6, P2=64, *, paths=4, subpixel=1, direction=-1, fb_check=0, check=False, return_status=False,
               adaptive_p2=0, d_min=None, runner_up=False, second_view=False, max_diff=256):
    """disp, minC = stereo_sgm(left, right, dMax) as fsgm_amd.stereo_sgm, on torch tensors on the GPU: left, right (H, W) uint8
    or a batch (N, H, W); disp (disparity * 256) and minC uint32 of the same shape, plus conf uint8 / disp2 uint32 with
    fb_check=1.  The outputs stay in HBM; the work is queued on the current stream.  adaptive_p2=1: edge-aware P2 on `left`.
    d_min: an integer starts the search range at that disparity (fsgm::stereo_sgm_range) and makes disp / disp2 int32 true
    disparities * 256 (disp2 INT32_MIN where invalid); the dtype follows the argument, not its value: None (fsgm::stereo_sgm)
    keeps the uint32 outputs, 0 gives the same values as int32.  runner_up=True (fsgm::stereo_sgm_ru) appends minC2 uint32, the
    runner-up cost min { S[d] : |d - best| >= 2 } (0xFFFFFFFF where no such d exists), to the outputs; the call then runs the
    line kernels at every batch size.  second_view=True (fsgm_view2::stereo_sgm; not with fb_check) appends disp2 int32, minC_v2
    uint32 and conf uint8 as fsgm_amd.stereo_sgm(second_view=True); disp is then int32 as with d_min (None: 0)."""
    d_min = _d_min(d_min)
    left, right, batched = _stereo_inputs(left, right, dMax, paths, subpixel, direction, fb_check, adaptive_p2)
    if second_view:
        if fb_check:
            raise ValueError("second_view=True and fb_check=1 are two different checks: ask for one")
        disp, minC, minC2, disp2, minC_v2, conf, status = torch.ops.fsgm_view2.stereo_sgm(
            left, right, int(dMax), d_min or 0, int(P1), int(P2), int(paths), int(subpixel), int(direction), int(adaptive_p2), bool(runner_up),
            int(max_diff))
        outs = (disp, minC) + ((minC2,) if runner_up else ()) + (disp2, minC_v2, conf)
        return _finish(outs, status, batched, check, return_status)
    rest = (int(P1), int(P2), int(paths), int(subpixel), int(direction), int(bool(fb_check)), int(adaptive_p2))
    if runner_up:
        disp, minC, minC2, conf, disp2, status = torch.ops.fsgm.stereo_sgm_ru(left, right, int(dMax), d_min or 0, *rest)
        if d_min is None:                                    # the uint32 outputs of the call without d_min (disp2: 512 << 8 where invalid)
            disp = disp.view(torch.uint32)
            if fb_check:
                disp2 = torch.where(disp2 == -2 ** 31, 512 << 8, disp2).view(torch.uint32)
    elif d_min is None:
        disp, minC, conf, disp2, status = torch.ops.fsgm.stereo_sgm(left, right, int(dMax), *rest)
    else:
        disp, minC, conf, disp2, status = torch.ops.fsgm.stereo_sgm_range(left, right, int(dMax), d_min, *rest)
    outs = ((disp, minC, conf, disp2) if fb_check else (disp, minC)) + ((minC2,) if runner_up else ())
    return _finish(outs, status, batched, check, return_status)


def view2_check(disp, disp2, *, direction=-1, max_diff=256):
    """conf = fsgm_amd.view2_check(disp, disp2) on torch tensors on the GPU (fsgm_view2::check): int32 true-disparity maps * 256,
    (H, W) or (N, H, W), disp2's marker INT32_MIN; conf uint8 of the same shape, queued on the current stream."""
    _tensors({"disp": (disp, torch.int32), "disp2": (disp2, torch.int32)})
    if disp.dim() not in (2, 3):
        raise TypeError(f"disp must be (H, W) or (N, H, W) (got {tuple(disp.shape)})")
    _shape("disp2", disp2, disp.shape)
    if int(direction) not in (-1, 1):
        raise ValueError(f"direction must be -1 or +1 (got {direction!r})")
    if int(max_diff) < 0:
        raise ValueError(f"max_diff must be >= 0 (got {max_diff!r})")
    batched = disp.dim() == 3
    if not batched:
        disp, disp2 = disp.unsqueeze(0), disp2.unsqueeze(0)
    conf, _ = torch.ops.fsgm_view2.check(disp, disp2, int(direction), int(max_diff))
    return conf if batched else conf[0]


def stereo_sgm_pp(left, right, dMax, P1=6, P2=64, *, paths=4, subpixel=1, direction=-1, adaptive_p2=0, d_min=0, in_fill=1, check=False,
                  return_status=False, **chain):
    """(disp_pp, disp_checked, disp, minC, disp2) as fsgm_amd.stereo_sgm_pp, on torch tensors on the GPU: left, right (H, W)
    uint8 or a batch (N, H, W).  The images are read where they lie, every output stays in HBM, the work is queued on the
    current stream.  disp_pp / disp_checked / disp2 float64, disp int32 (true disparity * 256), minC uint32."""
    d_min = _d_min(0 if d_min is None else d_min)
    left, right, batched = _stereo_inputs(left, right, dMax, paths, subpixel, direction, 0, adaptive_p2)
    defaults = _stereo_pp_params(_L, in_fill, chain)                        # (unknown names raise here)
    *outs, status = torch.ops.fsgm.stereo_sgm_pp(left, right, int(dMax), d_min, int(P1), int(P2), int(paths), int(subpixel), int(direction),
                                                 int(adaptive_p2), [float(getattr(defaults, k)) for k in STEREO_PP_FIELDS], int(in_fill))
    return _finish(outs, status, batched, check, return_status)


def uniqueness_filter(map, minC, minC2, ratio, *, planes=1):
    """fsgm_amd.uniqueness_filter on torch tensors on the GPU: map float64, minC / minC2 uint32 (stereo_sgm(runner_up=True)'s),
    (H, W) or (N, H, W); NaN where minC2 * (100 - ratio) < minC * 100 and minC2 is a runner-up, map elsewhere.  A new tensor;
    the work is queued on the current stream.  planes=2 (fsgm::uniqueness_filter_planes): map is a flow (2, H, W) or (N, 2, H, W)
    next to costs (H, W) / (N, H, W) -- sgm2d(runner_up=True)'s -- and both planes of a rejected pixel become NaN."""
    _tensors({"map": (map, torch.float64), "minC": (minC, torch.uint32), "minC2": (minC2, torch.uint32)})
    if isinstance(planes, bool) or planes not in (1, 2):
        raise ValueError(f"planes must be 1 or 2 (got {planes!r})")
    if planes == 2:
        if map.dim() not in (3, 4) or map.shape[-3] != 2:
            raise TypeError(f"map must be (2, H, W) or (N, 2, H, W) with planes=2 (got {tuple(map.shape)})")
        cshape = tuple(map.shape[:-3]) + tuple(map.shape[-2:])
    else:
        if map.dim() not in (2, 3):
            raise TypeError(f"map must be (H, W) or (N, H, W) (got {tuple(map.shape)})")
        cshape = tuple(map.shape)
    _shape("minC", minC, cshape)
    _shape("minC2", minC2, cshape)
    if isinstance(ratio, bool) or int(ratio) != ratio or not 0 <= int(ratio) <= 100:
        raise ValueError(f"ratio must be an integer in [0, 100] (got {ratio!r})")
    batched = len(cshape) == 3
    a, b, c = (map, minC, minC2) if batched else (map.unsqueeze(0), minC.unsqueeze(0), minC2.unsqueeze(0))
    if planes == 2:
        out, _ = torch.ops.fsgm.uniqueness_filter_planes(a, b, c, int(ratio), 2)
    else:
        out, _ = torch.ops.fsgm.uniqueness_filter(a, b, c, int(ratio))
    return out if batched else out[0]


def stereo_fb_check(D1, D2=None, d_min=0, direction=-1, thr=2.0, *, return_second=False, check=False, return_status=False):
    """fsgm_amd.stereo_fb_check on torch tensors on the GPU: D1 (and D2) (H, W) or (N, H, W) float64.  D2=None: the second-view
    map is made from D1 in the same kernel (return_second=True also returns it).  The status tensor (return_status=True) is
    FSGM_ERR_INVALID when that form met a negative D1 value; check=True synchronises and raises on it."""
    d_min = _d_min(d_min)
    named = {"D1": (D1, torch.float64)}
    if D2 is not None:
        named["D2"] = (D2, torch.float64)
    _tensors(named)
    if D1.dim() not in (2, 3):
        raise TypeError(f"D1 must be (H, W) or (N, H, W) (got {tuple(D1.shape)})")
    if D2 is not None:
        _shape("D2", D2, D1.shape)
        if return_second:
            raise ValueError("return_second needs D2=None")
    batched = D1.dim() == 3
    a = D1 if batched else D1.unsqueeze(0)
    b = a if D2 is None else (D2 if batched else D2.unsqueeze(0))
    out, second, status = torch.ops.fsgm.stereo_fb_check(a, b, int(D2 is None), d_min, int(direction), float(thr))
    outs = (out, second) if return_second else (out,)
    res = _finish(outs, status, batched, check, return_status, "a D1 value is negative")
    return res if return_second or return_status else res[0]


def _epipolar_inputs(I0, I1, F, H, epipole, direction):
    """(I0, I1 with a leading N, the ops' flat geometry list, batched) of the epipolar wrappers' arguments."""
    batched = np.asarray(F, dtype=np.float64).ndim == 3
    Fs, Hs, es, ds = (F, H, epipole, direction) if batched else ([F], [H], [epipole], [direction])
    if not (len(Fs) == len(Hs) == len(es) == len(ds)):
        raise ValueError("F, H, epipole and direction must hold one entry per frame")
    _tensors({"I0": (I0, torch.uint8), "I1": (I1, torch.uint8)})
    _shape("I1", I1, I0.shape)
    per = I0.dim() - (1 if batched else 0)
    if per not in (2, 3) or (per == 3 and I0.shape[-3] != 3):
        raise TypeError(f"images must be (H, W) or (3, H, W) per frame (got {tuple(I0.shape)})")
    if batched and I0.shape[0] != len(Fs):
        raise ValueError(f"{I0.shape[0]} image pairs but {len(Fs)} geometries")
    geometry = []
    for Fm, Hm, e, d in zip(Fs, Hs, es, ds):
        Fm, Hm = np.asarray(Fm, np.float64), np.asarray(Hm, np.float64)
        if Fm.shape != (3, 3) or Hm.shape != (3, 3):
            raise TypeError("F and H must be 3x3 matrices")
        geometry += [float(x) for x in Fm.reshape(-1)] + [float(x) for x in Hm.reshape(-1)]
        geometry += [float(e[0]), float(e[1]), float(bool(d))]
    if not batched:
        I0, I1 = I0.unsqueeze(0), I1.unsqueeze(0)
    return I0, I1, geometry, batched


def epipolar_sgm_of(I0, I1, F, H, epipole, direction, dMax=64, vMax=0.3, *, paths=4, check=False, return_status=False):
    """[flow, minC] = epipolar_sgm_of(...) as fsgm_amd.epipolar_sgm_of, on torch tensors on the GPU.  One frame: I0, I1
    (H, W) or RGB (3, H, W) uint8 with F, H (3x3), epipole (x, y), direction; a batch: images with a leading N and lists of N
    geometries (F then a sequence of 3x3 matrices).  flow (.., 3, H, W) float64, minC (.., H, W) uint32."""
    I0, I1, geometry, batched = _epipolar_inputs(I0, I1, F, H, epipole, direction)
    flow, minC, status = torch.ops.fsgm.epipolar_sgm_of(I0, I1, geometry, int(dMax), float(vMax), int(paths))
    return _finish((flow, minC), status, batched, check, return_status)


def epipolar_flow_pp(I0, I1, F, H, epipole, direction, dMax=64, vMax=0.3, *, paths=4, check=False, return_status=False):
    """(flow, flow2, D1, minC) of test.m's frame body as fsgm_amd.epipolar_flow_pp, on torch tensors on the GPU; images and
    geometries as epipolar_sgm_of.  flow / flow2 (.., 3, H, W) float64, D1 (.., H, W) float64, minC (.., H, W) uint32."""
    I0, I1, geometry, batched = _epipolar_inputs(I0, I1, F, H, epipole, direction)
    flow, flow2, D1, minC, status = torch.ops.fsgm.epipolar_flow_pp(I0, I1, geometry, int(dMax), float(vMax), int(paths))
    return _finish((flow, flow2, D1, minC), status, batched, check, return_status)


def epi_postprocess(D1, Pd0, normDirect, O, vMax, n, dMax, *, check=False, return_status=False):
    """test.m:45-50 as fsgm_amd.epi_postprocess(_batch), on torch tensors on the GPU.  One map: D1, O (H, W) and Pd0, normDirect
    (2, H, W) float64; a batch: the same with a leading N.  Returns (filterD1, filterD2, filterdisparites) float64 of D1's
    shape (the status tensor last with return_status=True: FSGM_ERR_INVALID when some D1 value is negative; check=True
    synchronises and raises on it)."""
    _tensors({"D1": (D1, torch.float64), "Pd0": (Pd0, torch.float64), "normDirect": (normDirect, torch.float64),
              "O": (O, torch.float64)})
    if D1.dim() not in (2, 3):
        raise TypeError(f"D1 must be (H, W) or (N, H, W) (got {tuple(D1.shape)})")
    batched = D1.dim() == 3
    lead = tuple(D1.shape[:-2])
    Hd, Wd = D1.shape[-2:]
    _shape("Pd0", Pd0, lead + (2, Hd, Wd))
    _shape("normDirect", normDirect, lead + (2, Hd, Wd))
    _shape("O", O, lead + (Hd, Wd))
    if not batched:
        D1, Pd0, normDirect, O = (t.unsqueeze(0) for t in (D1, Pd0, normDirect, O))
    f1, f2, disp, status = torch.ops.fsgm.epi_postprocess(D1, Pd0, normDirect, O, float(vMax), float(n), float(dMax))
    return _finish((f1, f2, disp), status, batched, check, return_status, "a D1 value is negative")


def vmf(flow):
    """flowMed = vmf(flow) as fsgm_amd.vmf, on a torch tensor on the GPU: (channels, H, W) float64 with 1..3 channels, or a
    batch (N, channels, H, W).  No status: the kernel has no failure to report."""
    _tensors({"flow": (flow, torch.float64)})
    if flow.dim() not in (3, 4) or not 1 <= flow.shape[-3] <= 3:
        raise TypeError(f"flow must be (1..3, H, W) or (N, 1..3, H, W) (got {tuple(flow.shape)})")
    if flow.dim() == 3:
        return torch.ops.fsgm.vmf(flow.unsqueeze(0))[0]
    return torch.ops.fsgm.vmf(flow)


def flow_level_hints(flow, size=3):
    """fsgm_amd.flow_level_hints on a torch tensor on the GPU: flow (2, H, W) or (N, 2, H, W) float64 -> the next finer level's
    hint map (.., 2, 2H, 2W).  No status: the kernel has no failure to report."""
    size = _level_median_of(size)
    _tensors({"flow": (flow, torch.float64)})
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise TypeError(f"flow must be (2, H, W) or (N, 2, H, W) (got {tuple(flow.shape)})")
    if flow.dim() == 3:
        return torch.ops.fsgm.flow_level_hints(flow.unsqueeze(0), size)[0]
    return torch.ops.fsgm.flow_level_hints(flow, size)


def _pyramid_images(I0, I1, batch):
    _tensors({"I0": (I0, torch.uint8), "I1": (I1, torch.uint8)})
    _shape("I1", I1, I0.shape)
    if batch is None:                                    # (3, H, W) is one RGB pair unless batch=True says three gray ones
        batch = I0.dim() == 4 or (I0.dim() == 3 and I0.shape[0] != 3)
    per = I0.dim() - (1 if batch else 0)
    if per not in (2, 3) or (per == 3 and I0.shape[-3] != 3):
        raise TypeError(f"images must be (H, W) or (3, H, W) per pair (got {tuple(I0.shape)}, batch={batch})")
    return (I0, I1, True) if batch else (I0.unsqueeze(0), I1.unsqueeze(0), False)


def _overrides(fields, defaults, overrides, name):
    for k in overrides:
        if k not in fields:
            raise TypeError(f"unknown {name} parameter {k!r}")
    return [int(overrides.get(k, getattr(defaults, k))) for k in fields]


def _pyramidal(ops, fields, default, name, I0, I1, numPyd, batch, check, return_status, runner_up, level_median, overrides):
    """pyramidal_sgm and pyramidal_sgm_ng: ops = the matcher's (plain, _ru, _lm) ops"""
    plain, ru, lm = ops
    level_median = _level_median_of(level_median)
    I0, I1, batched = _pyramid_images(I0, I1, batch)
    params = _overrides(fields, default(), overrides, name)
    if level_median:
        *outs, status = lm(I0, I1, int(numPyd), params, level_median, bool(runner_up))
        outs = outs if runner_up else outs[:2]               # (minC2 is the empty placeholder then)
    elif runner_up:
        *outs, status = ru(I0, I1, int(numPyd), params)
    else:
        *outs, status = plain(I0, I1, int(numPyd), params)
    return _finish(outs, status, batched, check, return_status)


def pyramidal_sgm(I0, I1, numPyd=5, *, batch=None, check=False, return_status=False, runner_up=False, level_median=0, **overrides):
    """(mv, minC) of level 1 of pyramidal_sgm(I0, I1, numPyd) as fsgm_amd.pyramidal_sgm, on torch tensors on the GPU (the per-level
    flows are not offered).  Images (H, W) or RGB (3, H, W) uint8, or a batch with a leading N; batch=None infers it (a 3-D tensor
    with 3 planes is one RGB pair).  mv (.., 2, H, W) float64, minC (.., H, W) uint32.  Keyword overrides as fsgm_amd.pyramidal_sgm.
    runner_up=True: (mv, minC, minC2) with level 1's runner-up cost (fsgm::pyramidal_sgm_ru).  level_median=3 or 5: the median
    between levels of fsgm_amd.pyramidal_sgm (fsgm::pyramidal_sgm_lm); it combines with runner_up."""
    return _pyramidal((torch.ops.fsgm.pyramidal_sgm, torch.ops.fsgm.pyramidal_sgm_ru, torch.ops.fsgm.pyramidal_sgm_lm), PYRAMID_FIELDS,
                      _L.fsgm_pyramid_params_default, "pyramidal_sgm", I0, I1, numPyd, batch, check, return_status, runner_up, level_median,
                      overrides)


def pyramidal_sgm_ng(I0, I1, numPyd=3, *, batch=None, check=False, return_status=False, runner_up=False, level_median=0, **overrides):
    """(flow, minC) of level 1 of the pyramidal loop around calc_pyd_cost_sgm_ng as fsgm_amd.pyramidal_sgm_ng, on torch tensors
    on the GPU; shapes and batch as pyramidal_sgm.  runner_up=True: (flow, minC, minC2) (fsgm::pyramidal_sgm_ng_ru).
    level_median=3 or 5: the median between levels (fsgm::pyramidal_sgm_ng_lm)."""
    return _pyramidal((torch.ops.fsgm.pyramidal_sgm_ng, torch.ops.fsgm.pyramidal_sgm_ng_ru, torch.ops.fsgm.pyramidal_sgm_ng_lm),
                      NG_PYRAMID_FIELDS, _L.fsgm_ng_pyramid_params_default, "pyramidal_sgm_ng", I0, I1, numPyd, batch, check, return_status,
                      runner_up, level_median, overrides)


def pyramidal_flow_pp(I0, I1, numPyd=None, matcher="pyd", *, median=0, batch=None, check=False, return_status=False,
                      uniqueness_ratio=None, level_median=0, **overrides):
    """(flow_pp, flow_checked, flow_fwd, flow_bwd, minC) as fsgm_amd.pyramidal_flow_pp, on torch tensors on the GPU; images and
    batch as pyramidal_sgm.  flow_pp (.., 3, H, W), the flows (.., 2, H, W) float64, minC (.., H, W) uint32.
    uniqueness_ratio=r: the five outputs plus minC2, with the uniqueness test ahead of the chain (fsgm::pyramidal_flow_pp_u).
    level_median=3 or 5: both directions run with the median between levels (fsgm::pyramidal_flow_pp_lm)."""
    level_median = _level_median_of(level_median)
    if matcher not in MATCHERS:
        raise ValueError(f"matcher must be 'pyd' or 'ng' (got {matcher!r})")
    I0, I1, batched = _pyramid_images(I0, I1, batch)
    defaults = _L.fsgm_flow_pp_params_default(MATCHERS[matcher])
    sub, fields = (defaults.ng, NG_PYRAMID_FIELDS) if matcher == "ng" else (defaults.pyd, PYRAMID_FIELDS)
    chain = [float(overrides.pop(k, getattr(defaults, k))) for k in FLOW_PP_FIELDS]
    params = _overrides(fields, sub, overrides, "pyramidal_flow_pp")
    args = (I0, I1, MATCHERS[matcher], int(sub.numPyd if numPyd is None else numPyd), params, chain, int(median))
    want = uniqueness_ratio is not None
    if level_median:
        *outs, status = torch.ops.fsgm.pyramidal_flow_pp_lm(*args, _uniqueness_ratio_of(uniqueness_ratio) if want else 0, want, level_median)
        outs = outs if want else outs[:5]                    # (minC2 is the empty placeholder then)
    elif want:
        *outs, status = torch.ops.fsgm.pyramidal_flow_pp_u(*args, _uniqueness_ratio_of(uniqueness_ratio))
    else:
        *outs, status = torch.ops.fsgm.pyramidal_flow_pp(*args)
    return _finish(outs, status, batched, check, return_status)


def flow_fb_check(f, b, thr=2.0):
    """fsgm_amd.flow_fb_check on torch tensors on the GPU: f, b (2, H, W) or (N, 2, H, W) float64.  No status: the kernel has no
    failure to report."""
    _tensors({"f": (f, torch.float64), "b": (b, torch.float64)})
    if f.dim() not in (3, 4) or f.shape[-3] != 2:
        raise TypeError(f"f must be (2, H, W) or (N, 2, H, W) (got {tuple(f.shape)})")
    _shape("b", b, f.shape)
    if f.dim() == 3:
        return torch.ops.fsgm.flow_fb_check(f.unsqueeze(0), b.unsqueeze(0), float(thr))[0]
    return torch.ops.fsgm.flow_fb_check(f, b, float(thr))


def run_tensors(plan, I1, I2, pd0, nd, off, *, check=False, return_status=False):
    """All `plan.batch` frames of an EpiPlan (fsgm_epi_plan_run_device) in the plan's aggregation mode and penalties
    (set_agg_mode / set_penalties): I1, I2 (N, H, W) uint8, pd0 / nd (N, 2, H, W), off (N, H, W) float64 on the plan's GPU,
    N = plan.batch.  Returns (bestD, minC) uint32 (N, H, W), plus (conf, bestD2) for plans made with fb_check=1."""
    dev = _tensors({"I1": (I1, torch.uint8), "I2": (I2, torch.uint8), "pd0": (pd0, torch.float64), "nd": (nd, torch.float64),
                    "off": (off, torch.float64)})
    if dev.index != plan.device:
        raise TypeError(f"the tensors are on {dev}, the plan on device {plan.device}")
    N, H, W = plan.batch, plan.H, plan.W
    for name, t, shape in (("I1", I1, (N, H, W)), ("I2", I2, (N, H, W)), ("pd0", pd0, (N, 2, H, W)), ("nd", nd, (N, 2, H, W)),
                           ("off", off, (N, H, W))):
        _shape(name, t, shape)
    I1, I2, pd0, nd, off = (_ready(t) for t in (I1, I2, pd0, nd, off))
    bestD, minC, conf, bestD2, status = _matcher_outputs(I1, plan.fb_check)
    P1, P2, vMax = plan.penalties
    e, o = _epi_structs(I1, I2, pd0, nd, off, W, H, plan.D, vMax, P1, P2, bestD, minC, conf if plan.fb_check else None,
                        bestD2 if plan.fb_check else None)
    _call(dev, _L.fsgm_epi_plan_run_device, plan._h, N, C.byref(e), C.byref(o), _stream(dev), _p(status))
    outs = (bestD, minC, conf, bestD2) if plan.fb_check else (bestD, minC)
    return _finish(outs, status, True, check, return_status)
