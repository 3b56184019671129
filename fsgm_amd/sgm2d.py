"""The 2-D matcher on batches of caller-supplied cost volumes (include/fsgm.h: fsgm_sgm2d_batch_host; the same call on torch
tensors in HBM is fsgm_amd.torch_ops.sgm2d): calc_pyd_cost_sgm's hinted-window aggregation, WTA and parabolas on volumes the
caller made, e.g. a correlation layer's (N, 81, H, W) for a 9x9 window.  The semantics are the MEX's, not sgm2d.m's."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .sgm import CostFormat, cost_format

LAYOUTS = {"hwd": 0, "dhw": 1, "dhw_yx": 2}      # FSGM_COST2D_LAYOUT_HWD / _DHW / _DHW_YX


class Sgm2dParams(C.Structure):
    _fields_ = [("diagonal", C.c_int32), ("totalPass", C.c_int32), ("adaptive_p2", C.c_int32), ("subpixel", C.c_int32),
                ("device", C.c_int32), ("layout", C.c_int32), ("cost_bound", C.c_int32), ("reserved", C.c_int32 * 5)]


def _bind(lib):
    vp, i32 = C.c_void_p, C.c_int32
    lib.fsgm_sgm2d_params_default.restype = Sgm2dParams
    head = [i32, vp, i32, i32, i32, i32, i32, i32, C.POINTER(Sgm2dParams), vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.fsgm_sgm2d_batch_host.argtypes = head
    lib.fsgm_sgm2d_device.argtypes = head + [vp, vp]
    if hasattr(lib, "fsgm_sgm2d_batch_host_ru"):                 # (an older build behind FSGM_LIB_PATH has none): minC2 after minC
        lib.fsgm_sgm2d_batch_host_ru.argtypes = head[:15] + [vp] + head[15:]
        lib.fsgm_sgm2d_device_ru.argtypes = head[:15] + [vp] + head[15:] + [vp, vp]
    if hasattr(lib, "fsgm_sgm2d_batch_host_exact"):              # (nor these): the _ru forms' argument lists, minC2 may be NULL
        lib.fsgm_sgm2d_batch_host_exact.argtypes = head[:15] + [vp] + head[15:]
        lib.fsgm_sgm2d_device_exact.argtypes = head[:15] + [vp] + head[15:] + [vp, vp]
    if hasattr(lib, "fsgm_sgm2d_float_dptr"):                    # (nor these): fmt behind C, minC2 may be NULL, exact a switch
        fhead = head[:2] + [C.POINTER(CostFormat)] + head[2:15] + [vp] + head[15:] + [i32]
        lib.fsgm_sgm2d_float_batch_host.argtypes = fhead
        lib.fsgm_sgm2d_float_dptr.argtypes = fhead + [vp, vp]
        lib.fsgm_pyd_plan_ingest_float_dptr.argtypes = [vp, i32, vp, C.POINTER(CostFormat), i32, i32, vp, vp]
    lib.fsgm_sgm2d_last_kernel.restype = C.c_char_p
    lib.fsgm_sgm2d_ingest_lds.argtypes = [i32, i32, i32, C.POINTER(C.c_uint64)]
    lib.fsgm_pyd_plan_ingest_cost_device.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    return lib


ARITHS = ("wrap", "exact")


def arith_exact(arith):
    """True for arith="exact", False for "wrap" (the MEX's unsigned char path costs)."""
    if arith not in ARITHS:
        raise ValueError(f"arith must be 'wrap' or 'exact' (got {arith!r})")
    return arith == "exact"


def layout_code(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwd', 'dhw' or 'dhw_yx' (got {layout!r})")
    return LAYOUTS[layout]


def params(lib, *, diagonal=1, total_pass=2, adaptive_p2=0, subpixel=1, device=0, layout="hwd", cost_bound=255):
    p = lib.fsgm_sgm2d_params_default()
    p.diagonal, p.totalPass, p.adaptive_p2, p.subpixel = int(diagonal), int(total_pass), int(adaptive_p2), int(subpixel)
    p.device, p.layout, p.cost_bound = int(device), layout_code(layout), int(cost_bound)
    return p


def shape_of(shape, layout, half_x, half_y):
    """(N or None, H, W, D) of a volume's or a batch's shape in that layout; D must be the window's candidate count."""
    if int(half_x) != half_x or int(half_y) != half_y or half_x < 0 or half_y < 0:
        raise ValueError(f"half_x / half_y must be non-negative integers (got {half_x!r}, {half_y!r})")
    D = (2 * int(half_x) + 1) * (2 * int(half_y) + 1)
    want = "(H, W, D) or (N, H, W, D)" if layout == "hwd" else "(D, H, W) or (N, D, H, W)"
    if len(shape) not in (3, 4):
        raise TypeError(f"costs must be {want} for layout {layout!r} (got {tuple(shape)})")
    n = None if len(shape) == 3 else int(shape[0])
    a, b, c = (int(v) for v in shape[-3:])
    H, W, d = (a, b, c) if layout == "hwd" else (b, c, a)
    if d != D:
        raise ValueError(f"costs {tuple(shape)} hold {d} candidates a pixel, the {2 * int(half_x) + 1} x {2 * int(half_y) + 1} window "
                         f"has {D} ({want} for layout {layout!r})")
    return n, H, W, D


def last_kernel():
    """The aggregation that this thread's last sgm2d_batch / torch_ops.sgm2d call ran: "rows", "rows/wide", "generic",
    "generic/wrap" or, with arith="exact", "generic/exact"."""
    return _bind(_lib.load()).fsgm_sgm2d_last_kernel().decode()


def ingest_lds(layout, half_x, half_y):
    """Bytes of LDS per workgroup of the kernel that brings volumes of this layout into a plan (no device needed)."""
    b = C.c_uint64()
    check(_bind(_lib.load()).fsgm_sgm2d_ingest_lds(layout_code(layout), int(half_x), int(half_y), C.byref(b)))
    return int(b.value)


def sgm2d_batch(costs, half_x, half_y, P1=6, P2=32, *, layout="dhw", hints=None, guide=None, cost_bound=255, diagonal=1, total_pass=2,
                adaptive_p2=0, subpixel=1, return_flow=False, return_sum=False, device=0, runner_up=False, arith="wrap"):
    """(bestD, minC[, minC2], mvSub[, flow][, S]) of the 2-D matcher on cost volumes the caller made: costs uint8 (N, D, H, W) for layout
    "dhw" (channel sx*Sy + sy, the reference's candidate order) or "dhw_yx" (channel sy*Sx + sx, the y-slow order correlation
    layers emit), (N, H, W, D) for "hwd" (candidate index sx*Sy + sy); one volume without the leading N.  The window is
    Sx x Sy = (2*half_x+1) x (2*half_y+1), candidate (sx, sy) the displacement (sx - half_x, sy - half_y) added to the hint.
    hints float64 (N, 2, mvH, mvW), at least as large as the image (None: zeros); guide uint8 (N, H, W), the first image, read
    with adaptive_p2=1.  bestD (the index sx*Sy + sy in every layout), minC uint32 (N, H, W); mvSub, flow float64 (N, 2, H, W),
    flow = hint + window offset + mvSub; S uint32 (N, H, W, D).  cost_bound (1..255): no cost is larger -- with
    cost_bound + P2 + max(P1, P2) <= 255 the non-wrapping kernels run; a volume above a bound below 255 is refused (status 1).
    runner_up=True (fsgm_sgm2d_batch_host_ru) returns minC2 uint32 (N, H, W) after minC: the smallest sum at a Chebyshev distance
    >= 2 from the winner, NO_RUNNER_UP where the window holds no such candidate -- what uniqueness_filter(flow, minC, minC2, ratio,
    planes=2) takes; every other output is that of the call without it.
    arith="exact" (fsgm_sgm2d_batch_host_exact): path costs as integers that are never narrowed -- the SGM recurrence itself where
    the default "wrap" reproduces the MEX's unsigned char overflow, i.e. whenever max(costs) + P2 + max(P1, P2) > 255 (inside that
    budget the two agree bit for bit).  P1 and P2 must lie in 0..255 (status 1); such a call runs "generic/exact" at every window
    and bound, and runner_up=True combines with it."""
    lib = _bind(_lib.load())
    exact = arith_exact(arith)
    layout_code(layout)
    costs = np.ascontiguousarray(costs)
    if costs.dtype != np.uint8:
        raise TypeError("costs must be uint8")
    n, H, W, D = shape_of(costs.shape, layout, half_x, half_y)
    N = 1 if n is None else n
    lead = () if n is None else (n,)
    mvW = mvH = 0
    if hints is not None:
        hints = np.ascontiguousarray(hints)
        if hints.dtype != np.float64 or hints.ndim != len(lead) + 3 or hints.shape[:-2] != lead + (2,):
            raise TypeError(f"hints must be float64 of shape {lead + (2, 'mvH', 'mvW')} (got {hints.dtype} {hints.shape})")
        mvH, mvW = hints.shape[-2:]
        if mvH < H or mvW < W:
            raise ValueError(f"hints ({mvH} x {mvW}) must be at least as large as the image ({H} x {W})")
    if guide is not None:
        guide = np.ascontiguousarray(guide)
        if guide.dtype != np.uint8 or guide.shape != lead + (H, W):
            raise TypeError(f"guide must be uint8 of shape {lead + (H, W)}")
    prm = params(lib, diagonal=diagonal, total_pass=total_pass, adaptive_p2=adaptive_p2, subpixel=subpixel, device=device, layout=layout,
                 cost_bound=cost_bound)
    bestD, minC = np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint32)
    mvSub = np.empty((N, 2, H, W), np.float64)
    flow = np.empty((N, 2, H, W), np.float64) if return_flow else None
    S = np.empty((N, H, W, D), np.uint32) if return_sum else None
    minC2 = np.empty((N, H, W), np.uint32) if runner_up else None
    if exact:
        check(lib.fsgm_sgm2d_batch_host_exact(N, ptr(costs), W, H, int(half_x), int(half_y), int(P1), int(P2), C.byref(prm), ptr(hints),
                                              mvW, mvH, ptr(guide), ptr(bestD), ptr(minC), ptr(minC2), ptr(mvSub), ptr(flow), ptr(S)))
    elif runner_up:
        check(lib.fsgm_sgm2d_batch_host_ru(N, ptr(costs), W, H, int(half_x), int(half_y), int(P1), int(P2), C.byref(prm), ptr(hints), mvW,
                                           mvH, ptr(guide), ptr(bestD), ptr(minC), ptr(minC2), ptr(mvSub), ptr(flow), ptr(S)))
    else:
        check(lib.fsgm_sgm2d_batch_host(N, ptr(costs), W, H, int(half_x), int(half_y), int(P1), int(P2), C.byref(prm), ptr(hints), mvW,
                                        mvH, ptr(guide), ptr(bestD), ptr(minC), ptr(mvSub), ptr(flow), ptr(S)))
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + (mvSub,) + ((flow,) if return_flow else ()) + ((S,) if return_sum else ())
    return outs if n is not None else tuple(o[0] for o in outs)


def sgm2d_batch_float(costs, half_x, half_y, scale, offset=0.0, P1=6, P2=32, *, layout="dhw", hints=None, guide=None, cost_bound=255,
                      diagonal=1, total_pass=2, adaptive_p2=0, subpixel=1, return_flow=False, return_sum=False, device=0, runner_up=False,
                      arith="wrap"):
    """sgm2d_batch on float costs (fsgm_sgm2d_float_batch_host): costs float32 or float16 in the shapes sgm2d_batch takes -- a
    correlation layer's (N, 81, H, W) for a 9x9 window -- each voxel quantised on the device to the byte
    clamp(rint(float32(c) * scale + offset), 0, cost_bound) (one float32 multiply, one float32 add, ties to even; a negative scale
    turns a correlation into a cost) and the u8 path run on those bytes: the outputs are those of sgm2d_batch on them with the same
    cost_bound, bit for bit.  A voxel that rounds below 0 or above cost_bound, or a NaN, refuses the volume (status 1, nothing
    written).  The aggregation is chosen from cost_bound as declared.  Everything else as sgm2d_batch."""
    lib = _bind(_lib.load())
    exact = arith_exact(arith)
    layout_code(layout)
    costs = np.ascontiguousarray(costs)
    if costs.dtype not in (np.float32, np.float16):
        raise TypeError(f"costs must be float32 or float16 (got {costs.dtype}); uint8 volumes go to sgm2d_batch")
    fmt = cost_format(costs.dtype, scale, offset)
    n, H, W, D = shape_of(costs.shape, layout, half_x, half_y)
    N = 1 if n is None else n
    lead = () if n is None else (n,)
    mvW = mvH = 0
    if hints is not None:
        hints = np.ascontiguousarray(hints)
        if hints.dtype != np.float64 or hints.ndim != len(lead) + 3 or hints.shape[:-2] != lead + (2,):
            raise TypeError(f"hints must be float64 of shape {lead + (2, 'mvH', 'mvW')} (got {hints.dtype} {hints.shape})")
        mvH, mvW = hints.shape[-2:]
        if mvH < H or mvW < W:
            raise ValueError(f"hints ({mvH} x {mvW}) must be at least as large as the image ({H} x {W})")
    if guide is not None:
        guide = np.ascontiguousarray(guide)
        if guide.dtype != np.uint8 or guide.shape != lead + (H, W):
            raise TypeError(f"guide must be uint8 of shape {lead + (H, W)}")
    prm = params(lib, diagonal=diagonal, total_pass=total_pass, adaptive_p2=adaptive_p2, subpixel=subpixel, device=device, layout=layout,
                 cost_bound=cost_bound)
    bestD, minC = np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint32)
    mvSub = np.empty((N, 2, H, W), np.float64)
    flow = np.empty((N, 2, H, W), np.float64) if return_flow else None
    S = np.empty((N, H, W, D), np.uint32) if return_sum else None
    minC2 = np.empty((N, H, W), np.uint32) if runner_up else None
    check(lib.fsgm_sgm2d_float_batch_host(N, ptr(costs), C.byref(fmt), W, H, int(half_x), int(half_y), int(P1), int(P2), C.byref(prm),
                                          ptr(hints), mvW, mvH, ptr(guide), ptr(bestD), ptr(minC), ptr(minC2), ptr(mvSub), ptr(flow), ptr(S),
                                          int(exact)))
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + (mvSub,) + ((flow,) if return_flow else ()) + ((S,) if return_sum else ())
    return outs if n is not None else tuple(o[0] for o in outs)
