"""Host-side mirror of the reference's calc_cost_sgm MEX interface (calc_cost_sgm.cpp:539-598,
called from epipolar_sgm_of.m:45), on top of the C ABI.

Array convention = the MEX's memory order (include/fsgm.h): what MATLAB passes as a
width x height column-major matrix is here a C-contiguous numpy array of shape (height, width);
width x height x 2 maps are (2, height, width).
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import EpiParams, EpiIn, EpiOut, check, ptr


def _u8img(a, name):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise TypeError(f"{name} must be a 2-D uint8 array (got {a.dtype}, ndim {a.ndim})")
    return np.ascontiguousarray(a)


def _f64(a, shape, name):
    a = np.asarray(a)
    if a.dtype != np.float64 or a.shape != shape:
        raise TypeError(f"{name} must be float64 of shape {shape} (got {a.dtype} {a.shape})")
    return np.ascontiguousarray(a)


def _params(paths, subpixel, vz_to_disp, device, fb_check=0):
    p = EpiParams()
    p.paths, p.subpixel, p.vz_to_disp, p.device = int(paths), int(subpixel), int(vz_to_disp), int(device)
    p.fb_check = int(fb_check)
    return p


def auto_pipeline(width, height, dMax, batch, paths=4, P1=6, P2=64, cmax=24, cus=256, adaptive_p2=0):
    """Which aggregation pipeline auto mode takes for `batch` frames of this shape (fsgm_epi_auto_pipeline): a pure function of
    its arguments and the FSGM_EPI_* environment, no device needed.  adaptive_p2=1: the line kernels at every batch size."""
    if adaptive_p2:
        o = _lib.options(adaptive_p2)
        return _lib.load().fsgm_epi_auto_pipeline_opts(int(width), int(height), int(dMax), int(batch), int(paths), int(P1), int(P2),
                                                       int(cmax), int(cus), C.byref(o)).decode()
    return _lib.load().fsgm_epi_auto_pipeline(int(width), int(height), int(dMax), int(batch), int(paths), int(P1), int(P2), int(cmax), int(cus)).decode()


def cost_kernels(width, height, dMax, sampling=_lib.SAMPLING_VZ):
    """Which kernels the cost stage of a width x height x dMax plan launches (fsgm_epi_cost_kernels): "costbox" /
    "stereo-costbox" for the fused kernel, "<raw>+<box>" with raw in px / vec4 / scalar / stereo and box in box16 / box4 / box1
    for the two-kernel form.  The launchers' own selector under the environment as it stands (FSGM_COST_FUSED, FSGM_BOX16), no
    device needed; raises FsgmError for a shape plan creation refuses."""
    buf = C.create_string_buffer(32)
    check(_lib.load().fsgm_epi_cost_kernels(int(width), int(height), int(dMax), int(sampling), buf, len(buf)))
    return buf.value.decode()


def calc_cost_sgm_batch(frames, dMax, vMax, P1, P2, *, paths=4, subpixel=1, vz_to_disp=1, device=0,
                        return_volumes=False, fb_check=0, devices=None, adaptive_p2=0):
    """frames: list of (I1, I2, pixelPosD0, normDir, offset) of one shape, processed concurrently.

    devices: a device list (sequence of HIP ordinals, or text "0,1,2" like FSGM_DEVICES) -- frame i runs on
    devices[i % len(devices)], one host thread per entry inside the library, no collective
    (fsgm_calc_cost_sgm_batch_devices_host); `device` is ignored then.  Results do not depend on the list.
    adaptive_p2=1: the reference's edge-aware large penalty (see calc_cost_sgm); not offered with a device list."""
    if devices is not None and adaptive_p2:
        raise ValueError("adaptive_p2 is not offered with a device list")
    lib = _lib.load()
    n = len(frames)
    if n == 0:
        return []
    ins, outs, keep, res = (EpiIn * n)(), (EpiOut * n)(), [], []
    H, W = np.asarray(frames[0][0]).shape
    D = int(dMax)
    for i, (I1, I2, pd0, nd, off) in enumerate(frames):
        I1, I2 = _u8img(I1, "I1"), _u8img(I2, "I2")
        if I1.shape != (H, W) or I2.shape != (H, W):
            raise ValueError("all images of a batch must share one shape")
        pd0 = _f64(pd0, (2, H, W), "pixelPosD0")
        nd = _f64(nd, (2, H, W), "normlizeDirection")
        off = _f64(off, (H, W), "offsetFromPosD0")
        bestD = np.zeros((H, W), np.uint32)
        minC = np.zeros((H, W), np.uint32)
        Cv = np.zeros((H, W, D), np.uint8) if return_volumes else None
        Sv = np.zeros((H, W, D), np.uint32) if return_volumes else None
        keep.append((I1, I2, pd0, nd, off))
        e = ins[i]
        e.I1, e.I2, e.width, e.height, e.dMax, e.vMax = ptr(I1), ptr(I2), W, H, D, float(vMax)
        e.pixelPosD0, e.normDir, e.offset, e.P1, e.P2 = ptr(pd0), ptr(nd), ptr(off), int(P1), int(P2)
        o = outs[i]
        conf = np.zeros((H, W), np.uint8) if fb_check else None
        bestD2 = np.zeros((H, W), np.uint32) if fb_check else None
        o.bestD, o.minC, o.C, o.S, o.conf, o.bestD2 = ptr(bestD), ptr(minC), ptr(Cv), ptr(Sv), ptr(conf), ptr(bestD2)
        r = (bestD, minC, Cv, Sv) if return_volumes else (bestD, minC)
        res.append(r + (conf, bestD2) if fb_check else r)
    prm = _params(paths, subpixel, vz_to_disp, device, fb_check)
    if devices is not None:
        nd, darr = _lib.device_array(devices)
        check(lib.fsgm_calc_cost_sgm_batch_devices_host(n, ins, outs, C.byref(prm), nd, darr))
    elif adaptive_p2:
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_calc_cost_sgm_batch_host_opts(n, ins, outs, C.byref(prm), C.byref(opt)))
    else:
        check(lib.fsgm_calc_cost_sgm_batch_host(n, ins, outs, C.byref(prm)))
    return res


def calc_cost_sgm(I1, I2, dMax, vMax, pixelPosD0, normlizeDirection, offsetFromPosD0, P1, P2, *,
                  paths=4, subpixel=1, vz_to_disp=1, device=0, return_volumes=False, fb_check=0, adaptive_p2=0):
    """[bestD, minC] = calc_cost_sgm(I1, I2, dMax, vMax, pixelPosD0, normlizeDirection,
    offsetFromPosD0, P1, P2)  -- same argument order and meaning as the MEX.

    Keyword arguments are the reference's compile-time switches (defaults = as shipped).
    fb_check=1 additionally returns (conf, bestD2): the forward-backward check the reference has
    commented out (calc_cost_sgm.cpp:482-536, :589-590).
    adaptive_p2=1 is `adpativeP2 = true` (:102): every path step uses P2 / 8 in place of P2 where I1 differs by more than 25
    between the pixel and its predecessor on the path (:68-72).
    """
    return calc_cost_sgm_batch([(I1, I2, pixelPosD0, normlizeDirection, offsetFromPosD0)], dMax, vMax, P1, P2,
                               paths=paths, subpixel=subpixel, vz_to_disp=vz_to_disp, device=device,
                               return_volumes=return_volumes, fb_check=fb_check, adaptive_p2=adaptive_p2)[0]


def calc_cost_sgm_linear_batch(frames, dMax, P1, P2, *, paths=4, subpixel=1, device=0, return_volumes=False, fb_check=0,
                               adaptive_p2=0):
    """frames: list of (I1, I2, pixelPosD0, normDir) of one shape through fsgm_calc_cost_sgm_linear_batch_host."""
    lib = _lib.load()
    n = len(frames)
    if n == 0:
        return []
    ins, outs, keep, res = (EpiIn * n)(), (EpiOut * n)(), [], []
    H, W = np.asarray(frames[0][0]).shape
    D = int(dMax)
    for i, (I1, I2, pd0, nd) in enumerate(frames):
        I1, I2 = _u8img(I1, "I1"), _u8img(I2, "I2")
        if I1.shape != (H, W) or I2.shape != (H, W):
            raise ValueError("all images of a batch must share one shape")
        pd0 = _f64(pd0, (2, H, W), "pixelPosD0")
        nd = _f64(nd, (2, H, W), "normlizeDirection")
        bestD, minC = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
        Cv = np.zeros((H, W, D), np.uint8) if return_volumes else None
        Sv = np.zeros((H, W, D), np.uint32) if return_volumes else None
        conf = np.zeros((H, W), np.uint8) if fb_check else None
        bestD2 = np.zeros((H, W), np.uint32) if fb_check else None
        keep.append((I1, I2, pd0, nd))
        e = ins[i]
        e.I1, e.I2, e.width, e.height, e.dMax, e.vMax = ptr(I1), ptr(I2), W, H, D, 0.0
        e.pixelPosD0, e.normDir, e.offset, e.P1, e.P2 = ptr(pd0), ptr(nd), None, int(P1), int(P2)
        o = outs[i]
        o.bestD, o.minC, o.C, o.S, o.conf, o.bestD2 = ptr(bestD), ptr(minC), ptr(Cv), ptr(Sv), ptr(conf), ptr(bestD2)
        r = (bestD, minC, Cv, Sv) if return_volumes else (bestD, minC)
        res.append(r + (conf, bestD2) if fb_check else r)
    prm = _params(paths, subpixel, 0, device, fb_check)
    if adaptive_p2:
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_calc_cost_sgm_linear_batch_host_opts(n, ins, outs, C.byref(prm), C.byref(opt)))
    else:
        check(lib.fsgm_calc_cost_sgm_linear_batch_host(n, ins, outs, C.byref(prm)))
    return res


def calc_cost_sgm_linear(I1, I2, dMax, pixelPosD0, normlizeDirection, P1, P2, *, paths=4, subpixel=1, fb_check=0, device=0,
                         return_volumes=False, adaptive_p2=0):
    """[bestD, minC] of calc_cost_sgm.cpp built without its line 4 (USE_VZIND): candidate d is sampled d pixels along the
    per-pixel direction (:368-375), bestD is the index * 256 and never converted.  I1, I2 (height, width) uint8, pixelPosD0 and
    normlizeDirection (2, height, width) float64 (1-based start positions, as for calc_cost_sgm).  fb_check=1 also returns
    (conf, bestD2) of the forward-backward check on bestD / 256 (:429-536).  adaptive_p2=1: the edge-aware P2 of :68-72."""
    return calc_cost_sgm_linear_batch([(I1, I2, pixelPosD0, normlizeDirection)], dMax, P1, P2, paths=paths, subpixel=subpixel,
                                      device=device, return_volumes=return_volumes, fb_check=fb_check, adaptive_p2=adaptive_p2)[0]


def _stereo_params(paths, subpixel, direction, fb_check, device):
    if int(direction) not in (-1, 1):
        raise ValueError(f"direction must be -1 (the match lies at x - d) or +1 (x + d), got {direction!r}")
    if int(paths) not in (4, 8):
        raise ValueError(f"paths must be 4 or 8 (got {paths!r})")
    p = _lib.StereoParams()
    p.paths, p.subpixel, p.fb_check, p.direction, p.device = int(paths), int(subpixel), int(bool(fb_check)), int(direction), int(device)
    return p


D_MIN_LIMIT = 1024                                             # FSGM_D_MIN_LIMIT


def _d_min(d_min):
    """d_min of the stereo wrappers as an int (None stays None), checked as the library checks it"""
    if d_min is None:
        return None
    try:
        whole = not isinstance(d_min, bool) and int(d_min) == d_min
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise TypeError(f"d_min must be an integer or None (got {d_min!r})")
    if abs(int(d_min)) > D_MIN_LIMIT:
        raise ValueError(f"|d_min| must be <= {D_MIN_LIMIT} (got {d_min!r})")
    return int(d_min)


def stereo_sgm(left, right, dMax, P1=6, P2=64, *, paths=4, subpixel=1, direction=-1, fb_check=0, device=0, adaptive_p2=0, d_min=None,
               runner_up=False, second_view=False, max_diff=256):
    """disp, minC = stereo_sgm(left, right, dMax): semi-global matching of a rectified pair.  left, right (height, width) uint8
    or a batch (N, height, width); disp uint32 = disparity * 256 (whole disparities with subpixel=0), minC uint32, of the
    images' shape.  direction=-1: `left` is the left view and its match in `right` lies at x - d; +1: at x + d.  fb_check=1
    also returns (conf, disp2): the reference's forward-backward check (threshold 2 on the * 256 values; dMax <= 511).
    adaptive_p2=1: edge-aware large penalty -- a path step across an intensity edge of `left` (a difference above 25 between
    the pixel and its predecessor on the path) pays P2 / 8 instead of P2 (calc_cost_sgm.cpp:68-72).
    d_min: an integer (|d_min| <= 1024, may be negative) starts the search range there -- the dMax candidates are the disparities
    d_min .. d_min + dMax - 1, sampled at clamp(x + direction * d) -- and disp / disp2 come back as int32 TRUE disparities * 256
    (disp2: INT32_MIN where invalid).  The dtype follows the argument, not its value: d_min=0 gives int32 arrays with the values
    of d_min=None, which takes the path and the uint32 outputs (disp2: 512 << 8 where invalid) this function always had.
    runner_up=True appends minC2 uint32 to the tuple: the runner-up cost min { S[d] : |d - best| >= 2 } of the winner-take-all
    (NO_RUNNER_UP where no such d exists), what uniqueness_filter() takes next to minC.  Such a call runs the line kernels at
    every batch size; disp, minC, conf and disp2 are those of the call without it.
    second_view=True (fsgm_stereo_sgm_view2_host; not with fb_check) appends disp2, minC_v2, conf: the second view's disparity from
    the same aggregated volume (include/fsgm.h, "Second view"), int32 true disparity * 256 with INT32_MIN where no candidate lies
    in the image, its cost uint32, and the left-right check uint8 (|disp - disp2| <= max_diff at the matched pixel, 1/256 units).
    disp then is int32 true disparity * 256 as with d_min (None: 0).  Such a call runs the line kernels at every batch size.
    With subpixel=0 disp stays 256 * d_min + the whole index (as without second_view) while disp2 is 256 * (d_min + index): conf is
    computed on the scaled first view, and view2_check applies to the pair only after disp has been scaled the same way."""
    d_min = _d_min(d_min)
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim not in (2, 3):
        raise TypeError(f"left / right must be uint8 arrays (height, width) or (N, height, width) (got {left.dtype} {left.shape})")
    if right.shape != left.shape:
        raise TypeError(f"right must have left's shape {left.shape} (got {right.shape})")
    if int(dMax) < 1:
        raise ValueError(f"dMax must be >= 1 (got {dMax!r})")
    prm = _stereo_params(paths, subpixel, direction, fb_check, device)
    lib = _lib.load()
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    H, W = left.shape[-2:]
    n = 1 if left.ndim == 2 else left.shape[0]
    if n == 0:
        raise ValueError("empty batch")
    dtype = np.uint32 if d_min is None else np.int32
    disp, minC = np.zeros(left.shape, dtype), np.zeros(left.shape, np.uint32)
    conf = np.zeros(left.shape, np.uint8) if fb_check else None
    disp2 = np.zeros(left.shape, dtype) if fb_check else None
    if second_view:
        from . import view2
        if fb_check:
            raise ValueError("second_view=True and fb_check=1 are two different checks: ask for one")
        view2.bind(lib)
        disp = np.zeros(left.shape, np.int32)
        minC2 = np.zeros(left.shape, np.uint32) if runner_up else None
        d2, mv, cf = np.zeros(left.shape, np.int32), np.zeros(left.shape, np.uint32), np.zeros(left.shape, np.uint8)
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_stereo_sgm_view2_host(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
                                             d_min or 0, int(max_diff), ptr(disp), ptr(minC), ptr(minC2), ptr(d2), ptr(mv), ptr(cf)))
        return (disp, minC) + ((minC2,) if runner_up else ()) + (d2, mv, cf)
    if runner_up:
        ranged = disp.view(np.int32), None if disp2 is None else disp2.view(np.int32)
        minC2 = np.zeros(left.shape, np.uint32)
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_stereo_sgm_host_ru(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
                                          d_min or 0, ptr(ranged[0]), ptr(minC), ptr(minC2), ptr(conf), ptr(ranged[1])))
        if d_min is None and fb_check:                       # the marker of the call without d_min
            disp2[ranged[1] == np.iinfo(np.int32).min] = 512 << 8
        return (disp, minC, conf, disp2, minC2) if fb_check else (disp, minC, minC2)
    if d_min is not None:
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_stereo_sgm_host_range(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
                                             d_min, ptr(disp), ptr(minC), ptr(conf), ptr(disp2)))
    elif adaptive_p2:
        opt = _lib.options(adaptive_p2)
        check(lib.fsgm_stereo_sgm_host_opts(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), C.byref(opt),
                                            ptr(disp), ptr(minC), ptr(conf), ptr(disp2)))
    else:
        check(lib.fsgm_stereo_sgm_host(n, ptr(left), ptr(right), W, H, int(dMax), int(P1), int(P2), C.byref(prm), ptr(disp), ptr(minC),
                                       ptr(conf), ptr(disp2)))
    return (disp, minC, conf, disp2) if fb_check else (disp, minC)


def stereo_last_kernel():
    """The aggregation pipeline this thread's last stereo_sgm call (numpy or torch form) ran, '' before the first."""
    return _lib.load().fsgm_stereo_sgm_last_kernel().decode()


NO_RUNNER_UP = 0xFFFFFFFF                                      # FSGM_NO_RUNNER_UP


def uniqueness_filter(map, minC, minC2, ratio, *, device=0, planes=1):
    """OpenCV's uniquenessRatio on the matcher's own costs: map float64 (values or NaN), minC and minC2 uint32
    (stereo_sgm(runner_up=True)'s, or EpiPlan.download() / download_runner_up()), all (height, width) or (N, height, width).
    Returns map with NaN where minC2 != NO_RUNNER_UP and minC2 * (100 - ratio) < minC * 100 (64-bit products); ratio is an
    integer in [0, 100], 0 rejects nothing.  planes=2: map is a flow, (2, height, width) or (N, 2, height, width) next to costs
    of (height, width) / (N, height, width) -- sgm2d_batch(runner_up=True)'s -- and both planes of a rejected pixel become NaN."""
    if isinstance(planes, bool) or planes not in (1, 2):
        raise ValueError(f"planes must be 1 or 2 (got {planes!r})")
    m = np.ascontiguousarray(map)
    if planes == 2:
        if m.dtype != np.float64 or m.ndim not in (3, 4) or m.shape[-3] != 2:
            raise TypeError(f"map must be a float64 flow (2, height, width) or (N, 2, height, width) with planes=2 (got {m.dtype} {m.shape})")
    elif m.dtype != np.float64 or m.ndim not in (2, 3):
        raise TypeError(f"map must be a float64 array (height, width) or (N, height, width) (got {m.dtype} {m.shape})")
    cshape = m.shape if planes == 1 else m.shape[:-3] + m.shape[-2:]
    c, c2 = np.ascontiguousarray(minC), np.ascontiguousarray(minC2)
    for name, a in (("minC", c), ("minC2", c2)):
        if a.dtype != np.uint32 or a.shape != cshape:
            raise TypeError(f"{name} must be uint32 of map's shape {cshape} (got {a.dtype} {a.shape})")
    if isinstance(ratio, bool) or int(ratio) != ratio or not 0 <= int(ratio) <= 100:
        raise ValueError(f"ratio must be an integer in [0, 100] (got {ratio!r})")
    if m.size == 0:
        raise ValueError("empty map")
    H, W = m.shape[-2:]
    out = np.empty_like(m)
    n = 1 if c.ndim == 2 else c.shape[0]
    if planes == 2:
        check(_lib.load().fsgm_uniqueness_filter_planes_host(n, ptr(m), ptr(c), ptr(c2), W, H, 2, int(ratio), ptr(out), int(device)))
    else:
        check(_lib.load().fsgm_uniqueness_filter_host(n, ptr(m), ptr(c), ptr(c2), W, H, int(ratio), ptr(out), int(device)))
    return out


def stereo_maps(width, height, direction=-1):
    """(pixelPosD0, normlizeDirection) that calc_cost_sgm_linear takes for what stereo_sgm computes: Pd0 = (x + 1, y + 1),
    direction (direction, 0)."""
    yy, xx = np.mgrid[0:int(height), 0:int(width)].astype(np.float64)
    pd0 = np.ascontiguousarray(np.stack([xx + 1.0, yy + 1.0]))
    nd = np.ascontiguousarray(np.stack([np.full_like(xx, float(direction)), np.zeros_like(xx)]))
    return pd0, nd


def sgm(Cvol, P1=7, P2=100, *, paths=4, device=0, return_sum=False):
    """[bestD, minC] = sgm(C, P1, P2): sgm.m's call shape (sgm.m:1, defaults :4-10; test.m:36 passes 6, 64) on the MEX's
    aggregation and WTA.  C: (height, width, dMax) uint8.  bestD = disparity index * 256 (MEX parabola).  MEX semantics
    (mod-256 path arithmetic, path start stores minimum 0), not sgm.m's saturating ones: see include/fsgm.h."""
    lib = _lib.load()
    Cvol = np.ascontiguousarray(Cvol)
    if Cvol.dtype != np.uint8 or Cvol.ndim != 3:
        raise TypeError("C must be a (height, width, dMax) uint8 array")
    H, W, D = Cvol.shape
    bestD, minC = np.empty((H, W), np.uint32), np.empty((H, W), np.uint32)
    S = np.empty((H, W, D), np.uint32) if return_sum else None
    check(lib.fsgm_sgm_host(ptr(Cvol), W, H, D, int(P1), int(P2), int(paths), ptr(bestD), ptr(minC), ptr(S), int(device)))
    return (bestD, minC, S) if return_sum else (bestD, minC)


def census(img, *, device=0):
    """census(img) of common.cpp:3-27 on the device: (height, width) uint8 -> uint32 codes."""
    lib = _lib.load()
    img = _u8img(img, "img")
    H, W = img.shape
    cen = np.empty((H, W), np.uint32)
    check(lib.fsgm_census_host(ptr(img), W, H, ptr(cen), int(device)))
    return cen


class EpiPlan:
    """Device-resident plan: `batch` frames of width x height x dMax stay in HBM across calls."""

    def __init__(self, width, height, dMax, batch=1, *, paths=4, subpixel=1, vz_to_disp=1, device=0, fb_check=0,
                 sampling=_lib.SAMPLING_VZ, direction=-1, adaptive_p2=0):
        """sampling: _lib.SAMPLING_VZ (the reference as shipped), SAMPLING_LINEAR (its build without USE_VZIND: upload() takes
        off=None) or SAMPLING_RECTIFIED (a rectified pair with match at x + direction * d: upload_images() only, no maps).
        adaptive_p2=1: set_adaptive_p2(1) on the fresh plan."""
        self.lib = _lib.load()
        self.W, self.H, self.D, self.batch, self.paths = int(width), int(height), int(dMax), int(batch), int(paths)
        self.device, self.fb_check = int(device), int(fb_check)
        self.penalties = (6, 64, 0.3)                        # (P1, P2, vMax) of a fresh plan (epipolar_sgm_of.m:16,19)
        self._h = C.c_void_p()
        self.sampling = int(sampling)
        prm = _params(paths, subpixel, vz_to_disp, device, fb_check)
        if self.sampling == _lib.SAMPLING_VZ:
            check(self.lib.fsgm_epi_plan_create(C.byref(self._h), self.W, self.H, self.D, self.batch, C.byref(prm)))
        else:
            check(self.lib.fsgm_epi_plan_create_sampling(C.byref(self._h), self.W, self.H, self.D, self.batch, C.byref(prm),
                                                         self.sampling, int(direction)))
        self.adaptive_p2 = 0
        self.runner_up = 0
        self.exact = 0
        self.d_min = 0
        if adaptive_p2:
            try:
                self.set_adaptive_p2(adaptive_p2)
            except Exception:
                self.close()
                raise

    def close(self):
        if self._h:
            self.lib.fsgm_epi_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_penalties(self, P1, P2, vMax=0.3):
        check(self.lib.fsgm_epi_plan_set_penalties(self._h, int(P1), int(P2), float(vMax)))
        self.penalties = (int(P1), int(P2), float(vMax))

    def set_agg_mode(self, mode):
        """0 auto, 1 per-direction line kernels, 2 fused pipeline when eligible, 3 parallel sweeps (8 paths) when eligible,
        4 band sweeps (all four paths of a pass in one sweep, one workgroup per frame: very large batches), 5 the same with the
        bands of a frame as workgroups of their own that hand over while they run (chained: batches from ~100 frames), 6 the
        parallel sweeps meeting in the middle (each finishes the other's half of the rows with the WTA inside: 10-25 frames)."""
        check(self.lib.fsgm_epi_plan_set_agg_mode(self._h, int(mode)))

    def set_adaptive_p2(self, on):
        """Adaptive P2 (calc_cost_sgm.cpp:68-72) on / off.  An adaptive plan runs the line kernels at every batch size:
        refused (status 4) while modes 2-6 are forced, as set_agg_mode(2..6) is on an adaptive plan; its aggregate stage reads
        I1 of every slot (upload / upload_images), also when the costs came from upload_cost."""
        check(self.lib.fsgm_epi_plan_set_adaptive_p2(self._h, int(on)))
        self.adaptive_p2 = int(on)

    def set_runner_up(self, on):
        """The WTA also writes the runner-up cost (download_runner_up) on / off.  Such a plan runs the line kernels at every batch
        size: refused (status 4) while modes 2-6 are forced, as set_agg_mode(2..6) is on such a plan.  Off: every output and
        every kernel selection is what it was."""
        check(self.lib.fsgm_epi_plan_set_runner_up(self._h, int(on)))
        self.runner_up = int(on)

    def set_exact(self, on):
        """Exact path arithmetic (include/fsgm.h, fsgm_sgm_batch_host_exact) on / off: path costs that are never narrowed to a
        byte, for costs and penalties outside the no-wrap budget.  Such a plan runs "packed16/exact" or "generic/exact" at every
        batch size and takes P1, P2 in 0..255 (status 1 otherwise): refused (status 4) while modes 2-6 are forced or the
        runner-up switch is on, as set_agg_mode(2..6) and set_runner_up(1) are on such a plan.  It composes with adaptive P2."""
        check(self.lib.fsgm_epi_plan_set_exact(self._h, int(on)))
        self.exact = int(on)

    def set_view2(self, on, direction=-1):
        """The second view (include/fsgm.h, "Second view") on / off: every WTA run also writes disp2 and minC_v2 (download_view2)
        from the same path volumes, candidate i of pixel x being second-view pixel x + direction * (d_min + i).  Such a plan runs
        the line kernels at every batch size; refused (status 4) on linear plans, on vz plans with vz_to_disp and while modes 2-6
        are forced; a rectified plan takes its own direction only (status 1)."""
        from . import view2
        check(view2.bind(self.lib).fsgm_epi_plan_set_view2(self._h, int(on), int(direction)))
        self.view2 = int(on)

    def download_view2(self, frame):
        """(disp2, minC_v2) uint32 of the last WTA run: index * 256 (+ parabola), view2.NO_VIEW2 where no candidate lies in the image."""
        from . import view2
        disp2, minC_v2 = np.empty((self.H, self.W), np.uint32), np.empty((self.H, self.W), np.uint32)
        check(view2.bind(self.lib).fsgm_epi_plan_download_view2(self._h, frame, ptr(disp2), ptr(minC_v2)))
        return disp2, minC_v2

    def set_d_min(self, d_min):
        """A rectified plan's search range starts at disparity d_min (|d_min| <= 1024; 0 at creation): candidate i is sampled at
        clamp(x + direction * (d_min + i)).  download() / download_fb() keep returning candidate indices * 256; any other plan
        refuses (status 4)."""
        check(self.lib.fsgm_epi_plan_set_d_min(self._h, int(d_min)))
        self.d_min = int(d_min)

    def upload(self, frame, I1, I2, pd0, nd, off):
        I1, I2 = _u8img(I1, "I1"), _u8img(I2, "I2")
        pd0 = _f64(pd0, (2, self.H, self.W), "pixelPosD0")
        nd = _f64(nd, (2, self.H, self.W), "normlizeDirection")
        off = None if off is None and self.sampling == _lib.SAMPLING_LINEAR else _f64(off, (self.H, self.W), "offsetFromPosD0")
        check(self.lib.fsgm_epi_plan_upload(self._h, frame, ptr(I1), ptr(I2), ptr(pd0), ptr(nd), ptr(off)))

    def upload_images(self, frame, I1, I2):
        I1, I2 = _u8img(I1, "I1"), _u8img(I2, "I2")
        if I1.shape != (self.H, self.W) or I2.shape != (self.H, self.W):
            raise TypeError(f"images must have shape {(self.H, self.W)}")
        check(self.lib.fsgm_epi_plan_upload_images(self._h, frame, ptr(I1), ptr(I2)))

    def upload_cost(self, frame, Cvol):
        Cvol = np.ascontiguousarray(Cvol)
        if Cvol.dtype != np.uint8 or Cvol.shape != (self.H, self.W, self.D):
            raise TypeError(f"C must be uint8 of shape {(self.H, self.W, self.D)}")
        check(self.lib.fsgm_epi_plan_upload_cost(self._h, frame, ptr(Cvol)))

    def copy_cost(self, dst, src, roll_cols=0):
        """Resident cost volume of frame dst <- frame src, columns rotated by roll_cols (device to device)."""
        check(self.lib.fsgm_epi_plan_copy_cost(self._h, int(dst), int(src), int(roll_cols)))

    def upload_offset(self, frame, off):
        off = _f64(off, (self.H, self.W), "offsetFromPosD0")
        check(self.lib.fsgm_epi_plan_upload_offset(self._h, frame, ptr(off)))

    def run(self, stages=_lib.STAGE_ALL):
        check(self.lib.fsgm_epi_plan_run(self._h, int(stages)))

    def sync(self):
        check(self.lib.fsgm_epi_plan_sync(self._h))

    def download(self, frame):
        bestD = np.empty((self.H, self.W), np.uint32)
        minC = np.empty((self.H, self.W), np.uint32)
        check(self.lib.fsgm_epi_plan_download(self._h, frame, ptr(bestD), ptr(minC)))
        return bestD, minC

    def download_fb(self, frame):
        """(conf, bestD2) of the forward-backward check (plans created with fb_check=1)."""
        conf = np.empty((self.H, self.W), np.uint8)
        bestD2 = np.empty((self.H, self.W), np.uint32)
        check(self.lib.fsgm_epi_plan_download_fb(self._h, frame, ptr(conf), ptr(bestD2)))
        return conf, bestD2

    def download_runner_up(self, frame):
        """minC2 of the last WTA run: min { S[d] : |d - best| >= 2 }, NO_RUNNER_UP where no such d exists (status 1 while the
        switch is off)."""
        minC2 = np.empty((self.H, self.W), np.uint32)
        check(self.lib.fsgm_epi_plan_download_runner_up(self._h, frame, ptr(minC2)))
        return minC2

    def download_cost(self, frame):
        Cv = np.empty((self.H, self.W, self.D), np.uint8)
        check(self.lib.fsgm_epi_plan_download_cost(self._h, frame, ptr(Cv)))
        return Cv

    def download_census(self, frame):
        """(cen1, cen2): the census codes FSGM_STAGE_COST computed for the two images (debug tap)."""
        c1 = np.empty((self.H, self.W), np.uint32)
        c2 = np.empty((self.H, self.W), np.uint32)
        check(self.lib.fsgm_epi_plan_download_census(self._h, frame, ptr(c1), ptr(c2)))
        return c1, c2

    def download_sum(self, frame):
        S = np.empty((self.H, self.W, self.D), np.uint32)
        check(self.lib.fsgm_epi_plan_download_sum(self._h, frame, ptr(S)))
        return S

    def time(self, stages, warmup=2, iters=10):
        ms = C.c_float()
        check(self.lib.fsgm_epi_plan_time(self._h, int(stages), int(warmup), int(iters), C.byref(ms)))
        return float(ms.value)

    def run_tensors(self, I1, I2, pd0, nd, off, **kw):
        """All frames of the plan from torch tensors on the GPU to torch tensors on the GPU, ordered on the current stream
        (fsgm_amd.torch_ops.run_tensors; import torch before the library is loaded)."""
        from . import torch_ops
        return torch_ops.run_tensors(self, I1, I2, pd0, nd, off, **kw)

    def ingest_cost(self, Cvol, **kw):
        """All frames' cost volumes from a uint8 torch tensor on the GPU, in either layout, ordered on the current stream
        (fsgm_amd.torch_ops.ingest_cost; import torch before the library is loaded)."""
        from . import torch_ops
        return torch_ops.ingest_cost(self, Cvol, **kw)

    @property
    def kernel_name(self):
        return self.lib.fsgm_epi_plan_kernel_name(self._h).decode()


# ---------------------------------------------------------------------------------------------
# epipolar driver, dense half (epipolar_geometry.m:99-115, rotation_motion.m, epipolar_sgm_of.m:33-51)
# ---------------------------------------------------------------------------------------------
class EpiGeometry(C.Structure):
    """What the sparse half of epipolar_geometry.m (:30-96, not built here) hands over."""
    _fields_ = [("F", C.c_double * 9), ("H", C.c_double * 9), ("epipole", C.c_double * 2), ("direction", C.c_int32)]


def _geometry(F, H, epipole, direction):
    F, H = np.asarray(F, np.float64), np.asarray(H, np.float64)
    if F.shape != (3, 3) or H.shape != (3, 3):
        raise TypeError("F and H must be 3x3 matrices")
    g = EpiGeometry()
    g.F[:] = list(F.reshape(-1))
    g.H[:] = list(H.reshape(-1))
    g.epipole[:] = [float(epipole[0]), float(epipole[1])]
    g.direction = int(bool(direction))
    return g


def _bind_driver(lib):
    if getattr(lib, "_epi_driver_bound", False):
        return
    vp, i32 = C.c_void_p, C.c_int32
    lib.fsgm_epipolar_maps_host.argtypes = [C.POINTER(EpiGeometry), i32, i32, vp, vp, vp, vp, i32]
    lib.fsgm_epipolar_sgm_of_host.argtypes = [vp, vp, i32, i32, i32, C.POINTER(EpiGeometry), i32, C.c_double,
                                              C.POINTER(_lib.EpiParams), vp, vp]
    lib.fsgm_epipolar_flow_pp_host.argtypes = [i32, vp, vp, i32, i32, i32, C.POINTER(EpiGeometry), i32, C.c_double,
                                               C.POINTER(_lib.EpiParams), vp, vp, vp, vp]
    lib._epi_driver_bound = True


def epipolar_from_F(F, K, pts1=None, pts2=None, inliers=None):
    """epipolar_geometry.m:40-96 on the host: (H, epipole, direction, ambiguous) from the fundamental matrix F, the intrinsics K
    and the matched points (n x 2 arrays of (x, y), MATLAB's 1-based pixel coordinates; inliers: boolean mask or None = all).
    What epipolar_maps / epipolar_sgm_of take next.  The SURF + LMedS estimate of F itself (:130-149) is toolbox code, not built."""
    lib = _lib.load()
    _bind_driver(lib)
    lib.fsgm_epipolar_from_F.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EpiGeometry), C.POINTER(C.c_int32)]
    F, K = np.ascontiguousarray(F, np.float64), np.ascontiguousarray(K, np.float64)
    if F.shape != (3, 3) or K.shape != (3, 3):
        raise TypeError("F and K must be 3x3 matrices")
    n = 0 if pts1 is None else len(pts1)
    p1 = np.ascontiguousarray(pts1, np.float64).reshape(n, 2) if n else None
    p2 = np.ascontiguousarray(pts2, np.float64).reshape(n, 2) if n else None
    inl = np.ascontiguousarray(inliers, np.uint8) if inliers is not None else None
    if inl is not None and inl.shape != (n,):
        raise ValueError("inliers must have one entry per match")
    g, amb = EpiGeometry(), C.c_int32()
    check(lib.fsgm_epipolar_from_F(ptr(F), ptr(K), n, ptr(p1), ptr(p2), ptr(inl), C.byref(g), C.byref(amb)))
    return np.array(g.H[:]).reshape(3, 3), (g.epipole[0], g.epipole[1]), int(g.direction), bool(amb.value)


def epipolar_maps(F, H, epipole, direction, width, height, *, device=0):
    """(PrefD0, NormlizeDirection, Offset, Rflow) of epipolar_geometry.m:99-115 from F, H = K*R/K, the
    epipole in image 2 and the expansion/contraction flag."""
    lib = _lib.load()
    _bind_driver(lib)
    g = _geometry(F, H, epipole, direction)
    Wd, Hd = int(width), int(height)
    Pd0, nd, rflow = (np.empty((2, Hd, Wd), np.float64) for _ in range(3))
    off = np.empty((Hd, Wd), np.float64)
    check(lib.fsgm_epipolar_maps_host(C.byref(g), Wd, Hd, ptr(Pd0), ptr(nd), ptr(off), ptr(rflow), int(device)))
    return Pd0, nd, off, rflow


def epipolar_sgm_of(I0, I1, F, H, epipole, direction, dMax=64, vMax=0.3, *, paths=4, device=0):
    """[flow, minC] = epipolar_sgm_of(I0, I1, K, dMax, vMax) from epipolar_sgm_of.m:33 on, with the sparse
    geometry (F, H, epipole, direction) given.  I0/I1: (height, width) or (3, height, width) uint8;
    flow: (3, height, width) float64, third plane 1."""
    lib = _lib.load()
    _bind_driver(lib)
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    if I0.dtype != np.uint8 or I1.dtype != np.uint8 or I0.shape != I1.shape:
        raise TypeError("I0/I1 must be uint8 images of one shape")
    if not (I0.ndim == 2 or (I0.ndim == 3 and I0.shape[0] == 3)):
        raise TypeError("images must be (height, width) or (3, height, width)")
    Hd, Wd = I0.shape[-2:]
    g = _geometry(F, H, epipole, direction)
    prm = _params(paths, 1, 1, device, 0)
    flow = np.empty((3, Hd, Wd), np.float64)
    minC = np.empty((Hd, Wd), np.uint32)
    check(lib.fsgm_epipolar_sgm_of_host(ptr(I0), ptr(I1), Wd, Hd, 1 if I0.ndim == 2 else 3, C.byref(g), int(dMax), float(vMax),
                                        C.byref(prm), ptr(flow), ptr(minC)))
    return flow, minC


def epipolar_flow_pp(I0, I1, F, H, epipole, direction, dMax=64, vMax=0.3, *, paths=4, device=0):
    """(flow, flow2, D1, minC) of test.m's frame body (:32-54) with the sparse geometry given: calc_cost_sgm in vz-index mode
    (P1 = 6, P2 = 64), D1 = bestD/256, flow (:38-42), the post-processing chain with n = dMax + 1 and flow2 (:50-54).
    One frame: I0/I1 (height, width) or (3, height, width) uint8 with F, H (3x3), epipole (x, y), direction; a batch: images
    with a leading N and lists of N geometries (F then a sequence of 3x3 matrices).  flow / flow2 (.., 3, height, width)
    float64 (third plane 1 where D1 / filterD1 is valid), D1 (.., height, width) float64, minC (.., height, width) uint32.
    D1 is the MEX's vz index (calc_cost_sgm's WTA); test.m's own comes from calc_cost.m + sgm.m."""
    lib = _lib.load()
    _bind_driver(lib)
    batched = np.asarray(F, dtype=np.float64).ndim == 3
    Fs, Hs, es, ds = (F, H, epipole, direction) if batched else ([F], [H], [epipole], [direction])
    if not (len(Fs) == len(Hs) == len(es) == len(ds)):
        raise ValueError("F, H, epipole and direction must hold one entry per frame")
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    if I0.dtype != np.uint8 or I1.dtype != np.uint8 or I0.shape != I1.shape:
        raise TypeError("I0/I1 must be uint8 images of one shape")
    if not batched:
        I0, I1 = I0[None], I1[None]
    if I0.shape[0] != len(Fs):
        raise ValueError(f"{I0.shape[0]} image pairs but {len(Fs)} geometries")
    if not (I0.ndim == 3 or (I0.ndim == 4 and I0.shape[1] == 3)):
        raise TypeError("images must be (height, width) or (3, height, width) per frame")
    N, (Hd, Wd) = I0.shape[0], I0.shape[-2:]
    g = (EpiGeometry * N)(*[_geometry(*x) for x in zip(Fs, Hs, es, ds)])
    prm = _params(paths, 1, 0, device, 0)
    flow, flow2 = np.empty((N, 3, Hd, Wd), np.float64), np.empty((N, 3, Hd, Wd), np.float64)
    D1, minC = np.empty((N, Hd, Wd), np.float64), np.empty((N, Hd, Wd), np.uint32)
    check(lib.fsgm_epipolar_flow_pp_host(N, ptr(I0), ptr(I1), Wd, Hd, 1 if I0.ndim == 3 else 3, g, int(dMax), float(vMax),
                                         C.byref(prm), ptr(flow), ptr(flow2), ptr(D1), ptr(minC)))
    outs = (flow, flow2, D1, minC)
    return outs if batched else tuple(o[0] for o in outs)
