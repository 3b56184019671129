"""sgm(C, P1, P2) on batches of caller-supplied cost volumes (include/fsgm.h: fsgm_sgm_batch_host; the same call on torch
tensors in HBM is fsgm_amd.torch_ops.sgm): either layout, a declared bound of the costs, every aggregation pipeline."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr

LAYOUTS = {"hwd": 0, "dhw": 1}          # FSGM_COST_LAYOUT_HWD / _DHW
COST_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}       # FSGM_COST_F32 / _F16 / _BF16


class SgmParams(C.Structure):
    _fields_ = [("paths", C.c_int32), ("subpixel", C.c_int32), ("device", C.c_int32), ("agg_mode", C.c_int32), ("layout", C.c_int32),
                ("cost_bound", C.c_int32), ("adaptive_p2", C.c_int32), ("reserved", C.c_int32 * 5)]


class CostFormat(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("scale", C.c_float), ("offset", C.c_float), ("reserved", C.c_int32 * 5)]


def cost_format(dtype, scale, offset=0.0):
    """fsgm_cost_format for a float volume: dtype "float32" / "float16" / "bfloat16" (or a numpy / torch dtype of that name); a
    voxel c becomes the byte clamp(rint(fp32(c) * scale + offset), 0, cost_bound), scale and offset rounded to float32 first
    (include/fsgm.h, "Float cost volumes").  The library refuses a zero or non-finite scale and a non-finite offset (status 1)."""
    try:
        name = np.dtype(dtype).name
    except TypeError:                                            # (a torch dtype, or "bfloat16", which numpy does not know)
        name = str(dtype).rsplit(".", 1)[-1]
    if name not in COST_DTYPES:
        raise TypeError(f"a float cost volume must be float32, float16 or bfloat16 (got {dtype})")
    f = CostFormat()
    f.dtype, f.scale, f.offset = COST_DTYPES[name], float(scale), float(offset)
    return f


def _bind(lib):
    vp, i32 = C.c_void_p, C.c_int32
    lib.fsgm_sgm_params_default.restype = SgmParams
    if hasattr(lib, "fsgm_sgm_float_dptr"):                      # (an older build behind FSGM_LIB_PATH has none): fmt behind C, exact a switch
        fmt = C.POINTER(CostFormat)
        lib.fsgm_cost_format_default.restype = CostFormat
        lib.fsgm_sgm_float_batch_host.argtypes = [i32, vp, fmt, i32, i32, i32, i32, i32, C.POINTER(SgmParams), vp, vp, vp, vp, vp, i32]
        lib.fsgm_sgm_float_dptr.argtypes = lib.fsgm_sgm_float_batch_host.argtypes + [vp, vp]
        lib.fsgm_epi_plan_ingest_float_dptr.argtypes = [vp, i32, vp, fmt, i32, i32, vp, vp]
    lib.fsgm_sgm_batch_host.argtypes = [i32, vp, i32, i32, i32, i32, i32, C.POINTER(SgmParams), vp, vp, vp, vp]
    lib.fsgm_sgm_device.argtypes = [i32, vp, i32, i32, i32, i32, i32, C.POINTER(SgmParams), vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "fsgm_sgm_batch_host_ru"):                   # (an older build behind FSGM_LIB_PATH has none): minC2 after minC
        lib.fsgm_sgm_batch_host_ru.argtypes = [i32, vp, i32, i32, i32, i32, i32, C.POINTER(SgmParams), vp, vp, vp, vp, vp]
        lib.fsgm_sgm_device_ru.argtypes = [i32, vp, i32, i32, i32, i32, i32, C.POINTER(SgmParams), vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "fsgm_sgm_batch_host_exact"):                # (nor these): the plain forms' argument lists
        lib.fsgm_sgm_batch_host_exact.argtypes = lib.fsgm_sgm_batch_host.argtypes
        lib.fsgm_sgm_device_exact.argtypes = lib.fsgm_sgm_device.argtypes
    lib.fsgm_sgm_last_kernel.restype = C.c_char_p
    lib.fsgm_sgm_ingest_lds.argtypes = [i32, i32, C.POINTER(C.c_uint64)]
    lib.fsgm_epi_plan_ingest_cost_device.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    return lib


ARITHS = ("mod256", "exact")


def arith_exact(arith):
    """True for arith="exact", False for "mod256" (the MEX's unsigned char path costs)."""
    if arith not in ARITHS:
        raise ValueError(f"arith must be 'mod256' or 'exact' (got {arith!r})")
    return arith == "exact"


def layout_code(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwd' or 'dhw' (got {layout!r})")
    return LAYOUTS[layout]


def params(lib, *, paths=4, subpixel=1, device=0, agg_mode=0, layout="hwd", cost_bound=255, adaptive_p2=0):
    p = lib.fsgm_sgm_params_default()
    p.paths, p.subpixel, p.device, p.agg_mode = int(paths), int(subpixel), int(device), int(agg_mode)
    p.layout, p.cost_bound, p.adaptive_p2 = layout_code(layout), int(cost_bound), int(adaptive_p2)
    return p


def shape_of(shape, layout):
    """(N or None, H, W, D) of a volume's or a batch's shape in that layout."""
    if len(shape) not in (3, 4):
        want = "(H, W, D) or (N, H, W, D)" if layout == "hwd" else "(D, H, W) or (N, D, H, W)"
        raise TypeError(f"C must be {want} for layout {layout!r} (got {tuple(shape)})")
    n = None if len(shape) == 3 else int(shape[0])
    a, b, c = (int(v) for v in shape[-3:])
    return (n, a, b, c) if layout == "hwd" else (n, b, c, a)


def last_kernel():
    """The pipeline that this thread's last sgm_batch / torch_ops.sgm call ran (EpiPlan.kernel_name's names)."""
    return _bind(_lib.load()).fsgm_sgm_last_kernel().decode()


def ingest_lds(layout, dMax):
    """Bytes of LDS per workgroup of the kernel that brings volumes of this layout into a plan (no device needed)."""
    b = C.c_uint64()
    check(_bind(_lib.load()).fsgm_sgm_ingest_lds(layout_code(layout), int(dMax), C.byref(b)))
    return int(b.value)


def sgm_batch(Cvol, P1=7, P2=100, *, paths=4, layout="hwd", cost_bound=255, agg_mode=0, adaptive_p2=0, guide=None, subpixel=1,
              return_sum=False, device=0, runner_up=False, arith="mod256", second_view=False, direction=-1, d_min=0, max_diff=256):
    """[bestD, minC] = sgm(C, P1, P2) (fsgm_amd.sgm) on a batch of volumes in one call, through one cached plan of that batch:
    C uint8 (N, H, W, D) for layout "hwd" or (N, D, H, W) for "dhw" (a cost-volume network's output; transposed on the device);
    one volume without the leading N.  bestD, minC uint32 (N, H, W); return_sum adds S uint32 (N, H, W, D).
    cost_bound (1..255): no cost is larger -- small bounds open the fused pipelines, as census costs do; a volume above a bound
    below 255 is refused (status 1).  agg_mode: EpiPlan.set_agg_mode's.  adaptive_p2=1 reads the edge-aware P2 from guide, the
    first image, uint8 (N, H, W).  runner_up=True (fsgm_sgm_batch_host_ru) returns minC2 uint32 (N, H, W) after minC, the
    runner-up cost min { S[d] : |d - best| >= 2 } (NO_RUNNER_UP where no such d exists): such a call runs the line kernels at
    every batch size (last_kernel() shows it), and agg_mode 2..6 with it is refused (status 4).
    arith="exact" (fsgm_sgm_batch_host_exact): path costs as integers that are never narrowed -- the SGM recurrence itself where
    the default "mod256" reproduces the MEX's unsigned char overflow, i.e. whenever max(C) + P2 + max(P1, P2) > 255 (inside that
    budget the two agree bit for bit).  P1 and P2 must lie in 0..255 (status 1); such a call runs "packed16/exact" or
    "generic/exact" at every batch size, agg_mode 2..6 with it is refused (status 4), and so is runner_up=True (ValueError).
    second_view=True (fsgm_sgm_view2_batch_host) appends disp2, minC_v2, conf: the second view's disparity from the same aggregated
    volume -- for second-view pixel x2 the first minimum over i of S[y][x2 - direction * (d_min + i)][i], uint32 index * 256 with
    the parabola like bestD, view2.NO_VIEW2 where no candidate lies in the image --, its cost uint32, and the left-right check
    uint8: 1 where the first view's match lands in the image on a valid disp2 that differs by at most max_diff (1/256 units).
    direction (-1 or +1) and d_min say that candidate i of pixel x is second-view pixel x + direction * (d_min + i).  Such a call
    runs the line kernels at every batch size; agg_mode 2..6 with it is refused (status 4); the other outputs are unchanged."""
    lib = _bind(_lib.load())
    exact = arith_exact(arith)
    if exact and runner_up:
        raise ValueError("arith='exact' has no runner-up cost: runner_up=True needs arith='mod256'")
    code = layout_code(layout)
    Cvol = np.ascontiguousarray(Cvol)
    if Cvol.dtype != np.uint8:
        raise TypeError("C must be uint8")
    n, H, W, D = shape_of(Cvol.shape, layout)
    N = 1 if n is None else n
    if guide is not None:
        guide = np.ascontiguousarray(guide)
        if guide.dtype != np.uint8 or guide.shape != (() if n is None else (n,)) + (H, W):
            raise TypeError(f"guide must be uint8 of shape {(() if n is None else (n,)) + (H, W)}")
    prm = params(lib, paths=paths, subpixel=subpixel, device=device, agg_mode=agg_mode, layout=layout, cost_bound=cost_bound,
                 adaptive_p2=adaptive_p2)
    assert prm.layout == code
    bestD, minC = np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint32)
    S = np.empty((N, H, W, D), np.uint32) if return_sum else None
    minC2 = np.empty((N, H, W), np.uint32) if runner_up else None
    if second_view:
        from . import view2
        view2.bind(lib)
        v2 = view2.params(lib, direction, d_min, max_diff)
        disp2, minC_v2, conf = np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint8)
        check(lib.fsgm_sgm_view2_batch_host(N, ptr(Cvol), W, H, D, int(P1), int(P2), C.byref(prm), C.byref(v2), ptr(guide), ptr(bestD),
                                            ptr(minC), ptr(minC2), ptr(S), int(exact), ptr(disp2), ptr(minC_v2), ptr(conf)))
        outs = (bestD, minC) + ((minC2,) if runner_up else ()) + ((S,) if return_sum else ()) + (disp2, minC_v2, conf)
        return outs if n is not None else tuple(o[0] for o in outs)
    if runner_up:
        check(lib.fsgm_sgm_batch_host_ru(N, ptr(Cvol), W, H, D, int(P1), int(P2), C.byref(prm), ptr(guide), ptr(bestD), ptr(minC),
                                         ptr(minC2), ptr(S)))
    elif exact:
        check(lib.fsgm_sgm_batch_host_exact(N, ptr(Cvol), W, H, D, int(P1), int(P2), C.byref(prm), ptr(guide), ptr(bestD), ptr(minC),
                                            ptr(S)))
    else:
        check(lib.fsgm_sgm_batch_host(N, ptr(Cvol), W, H, D, int(P1), int(P2), C.byref(prm), ptr(guide), ptr(bestD), ptr(minC), ptr(S)))
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + ((S,) if return_sum else ())
    return outs if n is not None else tuple(o[0] for o in outs)


def sgm_batch_float(costs, scale, offset=0.0, P1=7, P2=100, *, paths=4, layout="hwd", cost_bound=255, agg_mode=0, adaptive_p2=0, guide=None,
                    subpixel=1, return_sum=False, device=0, runner_up=False, arith="mod256"):
    """sgm_batch on float costs (fsgm_sgm_float_batch_host): costs float32 or float16 in the shapes sgm_batch takes, each voxel
    quantised on the device to the byte clamp(rint(float32(c) * scale + offset), 0, cost_bound) -- one float32 multiply, one
    float32 add, ties to even; a negative scale turns a similarity into a cost -- and the u8 path run on those bytes: the outputs
    are those of sgm_batch on them with the same cost_bound, bit for bit.  A voxel that rounds below 0 or above cost_bound, or a
    NaN, refuses the volume (status 1, nothing written).  The kernels are chosen from cost_bound as declared (no scan for the true
    maximum).  Everything else -- layout, agg_mode, adaptive_p2 / guide, runner_up, arith, return_sum -- as sgm_batch."""
    lib = _bind(_lib.load())
    exact = arith_exact(arith)
    if exact and runner_up:
        raise ValueError("arith='exact' has no runner-up cost: runner_up=True needs arith='mod256'")
    layout_code(layout)
    costs = np.ascontiguousarray(costs)
    if costs.dtype not in (np.float32, np.float16):
        raise TypeError(f"costs must be float32 or float16 (got {costs.dtype}); uint8 volumes go to sgm_batch")
    fmt = cost_format(costs.dtype, scale, offset)
    n, H, W, D = shape_of(costs.shape, layout)
    N = 1 if n is None else n
    if guide is not None:
        guide = np.ascontiguousarray(guide)
        if guide.dtype != np.uint8 or guide.shape != (() if n is None else (n,)) + (H, W):
            raise TypeError(f"guide must be uint8 of shape {(() if n is None else (n,)) + (H, W)}")
    prm = params(lib, paths=paths, subpixel=subpixel, device=device, agg_mode=agg_mode, layout=layout, cost_bound=cost_bound,
                 adaptive_p2=adaptive_p2)
    bestD, minC = np.empty((N, H, W), np.uint32), np.empty((N, H, W), np.uint32)
    S = np.empty((N, H, W, D), np.uint32) if return_sum else None
    minC2 = np.empty((N, H, W), np.uint32) if runner_up else None
    check(lib.fsgm_sgm_float_batch_host(N, ptr(costs), C.byref(fmt), W, H, D, int(P1), int(P2), C.byref(prm), ptr(guide), ptr(bestD), ptr(minC),
                                        ptr(minC2), ptr(S), int(exact)))
    outs = (bestD, minC) + ((minC2,) if runner_up else ()) + ((S,) if return_sum else ())
    return outs if n is not None else tuple(o[0] for o in outs)
