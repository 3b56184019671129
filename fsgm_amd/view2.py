"""The second view from the same aggregated volume and the left-right check against it (include/fsgm.h, "Second view"): the
ctypes side of fsgm_sgm_view2_*, fsgm_stereo_sgm_view2_* and fsgm_view2_check_*, behind sgm_batch(second_view=True),
stereo_sgm(second_view=True) and view2_check."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr

NO_VIEW2 = 0xFFFFFFFF                                            # FSGM_NO_VIEW2
INT32_MIN = -2 ** 31                                             # the stereo forms' marker


class View2Params(C.Structure):
    _fields_ = [("direction", C.c_int32), ("d_min", C.c_int32), ("max_diff", C.c_int32), ("reserved", C.c_int32 * 5)]


def bind(lib):
    from .sgm import SgmParams
    vp, i32 = C.c_void_p, C.c_int32
    v2, sgm, st, opt = C.POINTER(View2Params), C.POINTER(SgmParams), C.POINTER(_lib.StereoParams), C.POINTER(_lib.EpiOptions)
    lib.fsgm_view2_params_default.restype = View2Params
    lib.fsgm_sgm_view2_batch_host.argtypes = [i32, vp, i32, i32, i32, i32, i32, sgm, v2, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.fsgm_sgm_view2_dptr.argtypes = lib.fsgm_sgm_view2_batch_host.argtypes + [vp, vp]
    lib.fsgm_stereo_sgm_view2_host.argtypes = [i32, vp, vp, i32, i32, i32, i32, i32, st, opt, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.fsgm_stereo_sgm_view2_dptr.argtypes = lib.fsgm_stereo_sgm_view2_host.argtypes + [vp, vp]
    lib.fsgm_view2_check_host.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, i32]
    lib.fsgm_view2_check_dptr.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]
    lib.fsgm_view2_launch_lds.argtypes = [i32, C.POINTER(C.c_uint64)]
    lib.fsgm_view2_tile.argtypes = [i32]
    lib.fsgm_view2_tile.restype = i32
    lib.fsgm_epi_plan_set_view2.argtypes = [vp, i32, i32]
    lib.fsgm_epi_plan_download_view2.argtypes = [vp, i32, vp, vp]
    return lib


def params(lib, direction=-1, d_min=0, max_diff=256):
    p = lib.fsgm_view2_params_default()
    p.direction, p.d_min, p.max_diff = int(direction), int(d_min), int(max_diff)
    return p


def launch_lds(dMax):
    """Bytes of LDS a workgroup of the second view's kernel asks for at this dMax (no device needed)."""
    b = C.c_uint64()
    check(bind(_lib.load()).fsgm_view2_launch_lds(int(dMax), C.byref(b)))
    return int(b.value)


def tile(dMax):
    """Second-view pixels a workgroup of the tiled kernel owns at this dMax; 0: the generic kernel (dMax > 256)."""
    return int(bind(_lib.load()).fsgm_view2_tile(int(dMax)))


def view2_check(disp, disp2, *, direction=-1, max_diff=256, device=0):
    """conf = the left-right check on int32 true-disparity maps (* 256), (height, width) or (N, height, width), disp2's invalid
    marker INT32_MIN (stereo_sgm(second_view=True)'s outputs): conf[y][x] = 1 iff x2 = x + direction * ((disp + 128) >> 8) lies
    in the image, disp2[y][x2] is valid and |disp - disp2[y][x2]| <= max_diff (1/256 units, default one disparity)."""
    disp, disp2 = np.ascontiguousarray(disp), np.ascontiguousarray(disp2)
    if disp.dtype != np.int32 or disp2.dtype != np.int32 or disp.ndim not in (2, 3) or disp2.shape != disp.shape:
        raise TypeError("disp and disp2 must be int32 arrays of one shape, (height, width) or (N, height, width)")
    lib = bind(_lib.load())
    H, W = disp.shape[-2:]
    n = 1 if disp.ndim == 2 else disp.shape[0]
    conf = np.zeros(disp.shape, np.uint8)
    check(lib.fsgm_view2_check_host(n, ptr(disp), ptr(disp2), W, H, int(direction), int(max_diff), ptr(conf), int(device)))
    return conf
