"""Host-side mirror of the reference's pyramidal driver pyramidal_sgm.m (the MATLAB function around the
calc_pyd_cost_sgm MEX), on top of the C ABI: the whole level loop runs on the device.

Arrays follow the memory order the reference's drivers hand a MEX (after permute([2 1 3])): images
(height, width) or (3, height, width) uint8 C-contiguous, flows (2, height, width) float64, plane 0 = x.
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import check, ptr


class PyramidParams(C.Structure):
    _fields_ = [("numPyd", C.c_int32), ("P1", C.c_int32), ("P2", C.c_int32), ("aggHalfWinSize", C.c_int32),
                ("verSearchHalfWinSize", C.c_int32), ("horSearchHalfWinSize", C.c_int32), ("enableDiagonal", C.c_int32),
                ("totalPass", C.c_int32), ("adaptiveP2", C.c_int32), ("device", C.c_int32)]


class NgPyramidParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("numPyd", "P1", "P2", "halfSearchWinSize", "aggSize", "subPixelRefine", "device")]


_vp, _i32 = C.c_void_p, C.c_int32
# The plan functions that both matchers have, as _Plan._call names them: (suffix, arguments after the plan, the one-shot entry
# that came in the same build).  An older build behind FSGM_LIB_PATH has no "_ru" or no "_lm" entry and none of their rows.
_PLAN_FUNCTIONS = (("upload_frame", [_i32, _vp, _vp], ""), ("download_frame", [_i32, _i32, _vp, _vp], ""), ("destroy", [], ""),
                   ("level_size", [_i32, C.POINTER(_i32), C.POINTER(_i32)], ""), ("upload", [_vp, _vp], ""), ("run", [], ""),
                   ("download", [_i32, _vp, _vp], ""), ("time", [_i32, _i32, C.POINTER(C.c_float)], ""),
                   ("set_runner_up", [_i32], "_ru"), ("download_runner_up", [_i32, _vp], "_ru"), ("set_level_median", [_i32], "_lm"))


def _bind_matcher(lib, plan, host, Params):
    """What the two matchers declare alike: the plan functions `plan` + suffix and the one-shot entries `host`, `host`_ru, `host`_lm."""
    prm = C.POINTER(Params)
    getattr(lib, plan + "create").argtypes = [C.POINTER(_vp), _i32, _i32, _i32, prm]
    getattr(lib, plan + "destroy").restype = None
    images = [_vp, _vp, _i32, _i32, _i32, prm]
    getattr(lib, host).argtypes = images + [_vp, _vp, _vp]
    have = {"": True, "_ru": hasattr(lib, host + "_ru"), "_lm": hasattr(lib, host + "_lm")}
    if have["_ru"]:
        getattr(lib, host + "_ru").argtypes = images + [_vp, _vp, _vp, _vp]
    if have["_lm"]:
        getattr(lib, host + "_lm").argtypes = images + [_i32, _vp, _vp, _vp, _vp]
    for suffix, argtypes, since in _PLAN_FUNCTIONS:
        if have[since]:
            getattr(lib, plan + suffix).argtypes = [_vp] + argtypes


def _bind(lib):
    if getattr(lib, "_pyramid_bound", False):
        return
    lib.fsgm_pyramid_params_default.restype = PyramidParams
    _bind_matcher(lib, "fsgm_pyramid_plan_", "fsgm_pyramidal_sgm_host", PyramidParams)
    lib.fsgm_pyramid_plan_create_batch.argtypes = [C.POINTER(_vp), _i32, _i32, _i32, C.POINTER(PyramidParams), _i32]     # (prm, batch)
    lib.fsgm_pyramid_plan_run_images.argtypes = [_vp]
    lib.fsgm_pyramid_plan_sync.argtypes = [_vp]
    lib.fsgm_pyramid_plan_download_gray.argtypes = [_vp, _i32, _vp, _vp]
    lib.fsgm_pyramid_plan_download_gray_frame.argtypes = [_vp, _i32, _i32, _vp, _vp]
    if hasattr(lib, "fsgm_pyramidal_sgm_host_lm"):
        lib.fsgm_flow_level_hints_host.argtypes = [_i32, _vp, _i32, _i32, _i32, _vp, _i32]
    lib._pyramid_bound = True


def _bind_ng(lib):
    if getattr(lib, "_ng_pyramid_bound", False):
        return
    lib.fsgm_ng_pyramid_params_default.restype = NgPyramidParams
    _bind_matcher(lib, "fsgm_ng_pyramid_plan_", "fsgm_pyramidal_sgm_ng_host", NgPyramidParams)
    lib.fsgm_ng_pyramid_plan_create_batch.argtypes = [C.POINTER(_vp), _i32, _i32, _i32, _i32, C.POINTER(NgPyramidParams)]  # (batch, prm)
    lib._ng_pyramid_bound = True


def _params(default, numPyd, device, overrides, what):
    """The parameter struct default() returns, with numPyd, device and the keyword overrides (its field names) set."""
    prm = default()
    prm.numPyd, prm.device = int(numPyd), int(device)
    for k, v in overrides.items():
        if not hasattr(prm, k):
            raise TypeError(f"unknown {what} parameter {k!r}")
        setattr(prm, k, int(v))
    return prm


def _level_sizes(W, H, numPyd):
    """(width, height) of every level, finest first (impyramid: ceil(size / 2))."""
    sizes = [(W, H)]
    for _ in range(1, numPyd):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def _check_images(I0, I1):
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    if I0.dtype != np.uint8 or I1.dtype != np.uint8 or I0.shape != I1.shape:
        raise TypeError("I0/I1 must be uint8 images of one shape")
    if not (I0.ndim == 2 or (I0.ndim == 3 and I0.shape[0] == 3)):
        raise TypeError("images must be (height, width) or (3, height, width)")
    return I0, I1, (1 if I0.ndim == 2 else 3)


def level_median_of(size):
    """the window of the median between levels as the C ABI takes it: 0 (off), 3 or 5"""
    if isinstance(size, bool) or size not in (0, 3, 5):
        raise ValueError(f"level_median must be 0, 3 or 5 (got {size!r})")
    return int(size)


def _no_level_median_with_devices(kw):
    """the device-list forms have no level median (nor a runner-up cost)"""
    if kw.pop("level_median", 0):
        raise ValueError("level_median runs on one device: pass device= to the single-pair call, not devices=")


def flow_level_hints(flow, size=3, *, device=0):
    """The hint map the next finer pyramid level starts from: 2 * imresize(medfilt2(flow(:,:,c), [size size]), 2, 'nearest') per
    channel (pyramidal_sgm.m:70-72 with :70-71 live), the kernel the plans launch with level_median=size.  flow (2, height,
    width) float64 or a batch (N, 2, height, width); returns (.., 2, 2*height, 2*width).  size 0 is the plain doubling of :72.
    medfilt2 by vmf's rule: zero padding, the middle value of the sorted window, NaN above every number."""
    size = level_median_of(size)
    lib = _lib.load()
    _bind(lib)
    flow = np.ascontiguousarray(flow, np.float64)
    if flow.ndim not in (3, 4) or flow.shape[-3] != 2:
        raise TypeError(f"flow must be (2, height, width) or (N, 2, height, width) (got {flow.shape})")
    H, W = flow.shape[-2:]
    nxt = np.empty(flow.shape[:-2] + (2 * H, 2 * W), np.float64)
    check(lib.fsgm_flow_level_hints_host(1 if flow.ndim == 3 else flow.shape[0], ptr(flow), W, H, size, ptr(nxt), int(device)))
    return nxt


def _entry(lib, plain, second, level_median, minC2, ratio=()):
    """The C entry of a one-shot call, chosen by the newer switches: (function, its integers after the parameter struct, its minC2
    argument after minC), the last two as tuples to splice into the plain entry's arguments.  With every switch off that is the
    entry `plain` and nothing more, so such a call runs on an older build (FSGM_LIB_PATH) too; a runner-up cost alone -- minC2
    an array -- takes `plain` + `second` ("_ru", or "_u" with the flow chain's `ratio` = (r,)); level_median takes "_lm", where
    minC2 may be None (NULL)."""
    if level_median:
        return getattr(lib, plain + "_lm"), ratio + (level_median,), (ptr(minC2),)
    if minC2 is not None:
        return getattr(lib, plain + second), ratio, (ptr(minC2),)
    return getattr(lib, plain), (), ()


def _outputs(out, sizes, runner_up, coarsest_first):
    """(mv, the per-level flows finest first, minC, minC2 or None) of a one-shot call: new arrays, or those of out=, a previous
    call's result tuple (its level list coarsest first or not), when they are what this call writes."""
    W, H = sizes[0]
    if out is None:                                          # every element is written by the call
        return (np.empty((2, H, W), np.float64), [np.empty((2, h, w), np.float64) for (w, h) in sizes], np.empty((H, W), np.uint32),
                np.empty((H, W), np.uint32) if runner_up else None)
    mv, levels, minC, *minC2 = out
    if coarsest_first:
        levels = list(levels)[::-1]
    flows = [(mv, (W, H))] + list(zip(levels, sizes))
    ok = (len(minC2) == (1 if runner_up else 0) and len(levels) == len(sizes)
          and all(a.shape == (2, h, w) and a.dtype == np.float64 and a.flags.c_contiguous for a, (w, h) in flows)
          and all(a.shape == (H, W) and a.dtype == np.uint32 and a.flags.c_contiguous for a in [minC] + minC2))
    if not ok:
        raise ValueError("out does not match this call's shapes")
    return mv, levels, minC, (minC2[0] if runner_up else None)


def _one_shot(bind, default, stem, what, coarsest_first, I0, I1, numPyd, device, out, runner_up, level_median, overrides):
    """pyramidal_sgm and pyramidal_sgm_ng: `stem` names the C entries (stem + "_host", "_host_ru", "_host_lm"), `default` the
    function of the default parameters, `what` the call in messages; the level list is returned, and taken in out=, coarsest
    first or finest first."""
    level_median = level_median_of(level_median)
    lib = _lib.load()
    bind(lib)
    I0, I1, ch = _check_images(I0, I1)
    H, W = I0.shape[-2:]
    prm = _params(getattr(lib, default), numPyd, device, overrides, what)
    mv, levels, minC, minC2 = _outputs(out, _level_sizes(W, H, prm.numPyd), runner_up, coarsest_first)
    ptrs = (C.c_void_p * len(levels))(*[a.ctypes.data for a in levels])
    fn, switches, second = _entry(lib, stem + "_host", "_ru", level_median, minC2)
    check(fn(ptr(I0), ptr(I1), W, H, ch, C.byref(prm), *switches, ptr(mv), ptr(minC), *second, ptrs))
    return (mv, levels[::-1] if coarsest_first else levels, minC) + ((minC2,) if runner_up else ())


def pyramidal_sgm(I0, I1, numPyd=5, *, device=0, out=None, runner_up=False, level_median=0, **overrides):
    """[mvCurLevel, mvPyd, minC] = pyramidal_sgm(I0, I1, numPyd) (pyramidal_sgm.m:1).  runner_up=True: (mv, mvPyd, minC, minC2)
    with level 1's runner-up cost minC2 uint32 (height, width) (include/fsgm.h, the 2-D rule).  Keyword overrides
    name the function's hard-coded parameters (P1, P2, aggHalfWinSize, verSearchHalfWinSize,
    horSearchHalfWinSize, enableDiagonal, totalPass, adaptiveP2; pyramidal_sgm.m:15-22).
    out: a previous call's result tuple to write into instead of allocating (the results of that call are overwritten): a loop
    over frames then hands the library pages that are already resident, as a MEX gateway's zero-filled outputs are.
    level_median=3 or 5: every level's flow is median-filtered (medfilt2 with that window, pyramidal_sgm.m:70-71 live) on its way to
    the next finer level's hints; the returned flows stay unfiltered.  It combines with runner_up."""
    return _one_shot(_bind, "fsgm_pyramid_params_default", "fsgm_pyramidal_sgm", "pyramidal_sgm", False, I0, I1, numPyd, device, out,
                     runner_up, level_median, overrides)


class PyramidPair(C.Structure):
    _fields_ = [("I0", C.c_void_p), ("I1", C.c_void_p), ("mv", C.c_void_p), ("minC", C.c_void_p), ("mvPyd", C.c_void_p)]


def _pairs_over_devices(fn, prm, pairs, devices):
    """pairs of one shape through fsgm_pyramidal_sgm(_ng)_batch_devices_host: pair i on devices[i % len(devices)]."""
    n = len(pairs)
    arr, keep, res = (PyramidPair * n)(), [], []
    shape = None
    for i, (I0, I1) in enumerate(pairs):
        I0, I1, ch = _check_images(I0, I1)
        H, W = I0.shape[-2:]
        if shape not in (None, (W, H, ch)):
            raise ValueError("all pairs of a batch must share one shape")
        shape = (W, H, ch)
        sizes = _level_sizes(W, H, prm.numPyd)
        mv, minC = np.zeros((2, H, W), np.float64), np.zeros((H, W), np.uint32)
        lv = [np.zeros((2, h, w), np.float64) for (w, h) in sizes]
        ptrs = (C.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        arr[i].I0, arr[i].I1, arr[i].mv, arr[i].minC = ptr(I0), ptr(I1), ptr(mv), ptr(minC)
        arr[i].mvPyd = C.cast(ptrs, C.c_void_p)
        keep.append((I0, I1, ptrs))
        res.append((mv, lv, minC))
    nd, darr = _lib.device_array(devices)
    W, H, ch = shape
    check(fn(n, arr, W, H, ch, C.byref(prm), nd, darr))
    return res


def pyramidal_sgm_batch(pairs, numPyd=5, *, devices=(0,), **overrides):
    """pyramidal_sgm for a list of (I0, I1) pairs of one shape, pair i on devices[i % len(devices)] (one host thread per
    entry inside the library, no collective); returns a list of (mvCurLevel, mvPyd, minC) like pyramidal_sgm."""
    _no_level_median_with_devices(overrides)
    lib = _lib.load()
    _bind(lib)
    lib.fsgm_pyramidal_sgm_batch_devices_host.argtypes = [C.c_int32, C.POINTER(PyramidPair), C.c_int32, C.c_int32, C.c_int32,
                                                          C.POINTER(PyramidParams), C.c_int32, C.POINTER(C.c_int32)]
    prm = _params(lib.fsgm_pyramid_params_default, numPyd, 0, overrides, "pyramidal_sgm")
    return _pairs_over_devices(lib.fsgm_pyramidal_sgm_batch_devices_host, prm, pairs, devices)


class _Plan:
    """Device-resident pyramid for one image shape: upload a pair, run, download any level.  A subclass names its C functions'
    prefix (_prefix) and creates the plan (_create)."""
    _prefix = None

    def __init__(self, bind, default, what, width, height, channels, numPyd, device, batch, overrides):
        self.lib = _lib.load()
        bind(self.lib)
        self.prm = _params(getattr(self.lib, default), numPyd, device, overrides, what)
        self.W, self.H, self.channels, self.batch = int(width), int(height), int(channels), int(batch)
        self._h = C.c_void_p()
        check(self._create())

    def _call(self, name, *args):
        return getattr(self.lib, self._prefix + name)(self._h, *args)

    def close(self):
        if self._h:
            self._call("destroy")
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

    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        check(self._call("level_size", int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def upload(self, I0, I1, frame=0):
        I0, I1, ch = _check_images(I0, I1)
        if ch != self.channels or I0.shape[-2:] != (self.H, self.W):
            raise ValueError("shape mismatch with the plan")
        check(self._call("upload_frame", int(frame), ptr(I0), ptr(I1)))

    def run(self):
        check(self._call("run"))

    def download(self, level=1, frame=0):
        w, h = self.level_size(level)
        flow = np.empty((2, h, w), np.float64)
        minC = np.empty((h, w), np.uint32)
        check(self._call("download_frame", int(frame), int(level), ptr(flow), ptr(minC)))
        return flow, minC

    def set_runner_up(self, on=True):
        """Level 1's WTA also writes the runner-up cost minC2 (include/fsgm.h, the matcher's own rule); nothing else changes."""
        check(self._call("set_runner_up", 1 if on else 0))

    def set_level_median(self, size):
        """The median between levels: 0 (off), 3 or 5 -- medfilt2's window on each level's flow on its way to the next finer level's
        hints (pyramidal_sgm.m:70-71 live).  download() keeps returning the unfiltered flows.  Toggled freely between runs."""
        check(self._call("set_level_median", level_median_of(size)))

    def download_runner_up(self, frame=0):
        """minC2 uint32 (height, width) of level 1 of the last run; refused while the switch is off."""
        minC2 = np.empty((self.H, self.W), np.uint32)
        check(self._call("download_runner_up", int(frame), ptr(minC2)))
        return minC2

    def time(self, warmup=1, iters=5):
        ms = C.c_float()
        check(self._call("time", int(warmup), int(iters), C.byref(ms)))
        return float(ms.value)


class PyramidPlan(_Plan):
    """Device-resident pyramid for one image shape: upload a pair, run, download any level."""
    _prefix = "fsgm_pyramid_plan_"

    def __init__(self, width, height, channels=1, numPyd=5, *, device=0, batch=1, **overrides):
        super().__init__(_bind, "fsgm_pyramid_params_default", "pyramidal_sgm", width, height, channels, numPyd, device, batch, overrides)

    def _create(self):
        return self.lib.fsgm_pyramid_plan_create_batch(C.byref(self._h), self.W, self.H, self.channels, C.byref(self.prm), self.batch)

    def sync(self):
        """Wait for the queued work; plans started with run() before any sync() overlap on the device."""
        check(self._call("sync"))

    def run_images(self):
        """Only impyramid / rgb2gray (the level images), no matching."""
        check(self._call("run_images"))

    def download_gray(self, level=1, frame=0):
        """The gray image pair calc_pyd_cost_sgm saw at `level` (after impyramid / rgb2gray), of pair `frame` of the batch."""
        w, h = self.level_size(level)
        g0, g1 = np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)
        check(self._call("download_gray_frame", int(frame), int(level), ptr(g0), ptr(g1)))
        return g0, g1


class NgPyramidPlan(_Plan):
    """Device-resident level loop around calc_pyd_cost_sgm_ng for one image shape (see pyramidal_sgm_ng); `batch` image
    pairs stay resident and go through every level together."""
    _prefix = "fsgm_ng_pyramid_plan_"

    def __init__(self, width, height, channels=1, numPyd=3, *, device=0, batch=1, **overrides):
        super().__init__(_bind_ng, "fsgm_ng_pyramid_params_default", "pyramidal_sgm_ng", width, height, channels, numPyd, device, batch,
                         overrides)

    def _create(self):
        return self.lib.fsgm_ng_pyramid_plan_create_batch(C.byref(self._h), self.W, self.H, self.channels, self.batch, C.byref(self.prm))


def pyramidal_sgm_ng_batch(pairs, numPyd=3, *, devices=(0,), **overrides):
    """pyramidal_sgm_ng for a list of (I0, I1) pairs of one shape, pair i on devices[i % len(devices)]; returns a list of
    (flow of level 1, [flow per level], minC of level 1) like pyramidal_sgm_ng."""
    _no_level_median_with_devices(overrides)
    lib = _lib.load()
    _bind_ng(lib)
    lib.fsgm_pyramidal_sgm_ng_batch_devices_host.argtypes = [C.c_int32, C.POINTER(PyramidPair), C.c_int32, C.c_int32, C.c_int32,
                                                             C.POINTER(NgPyramidParams), C.c_int32, C.POINTER(C.c_int32)]
    prm = _params(lib.fsgm_ng_pyramid_params_default, numPyd, 0, overrides, "pyramidal_sgm_ng")
    return _pairs_over_devices(lib.fsgm_pyramidal_sgm_ng_batch_devices_host, prm, pairs, devices)


def pyramidal_sgm_ng(I0, I1, numPyd=3, *, device=0, out=None, runner_up=False, level_median=0, **overrides):
    """The level loop of pyramidal_sgm.m (:24-76) with calc_pyd_cost_sgm_ng swapped in for calc_pyd_cost_sgm
    (BASELINE config 4): the neighbour-guided MEX takes the previous level's flow as its hint map and returns
    the flow itself (calc_pyd_cost_sgm_ng.cpp:458-480).  Defaults are the argument values of ng_sgm.m:20
    (halfSearchWinSize=1, aggSize=2, subPixelRefine=0, P1=6, P2=32); keyword overrides name them.  Level images
    by impyramid 'reduce' / rgb2gray, hints of a finer level = 2*imresize(flow, 2, 'nearest') (pyramidal_sgm.m:72);
    everything stays on the device between levels.

    Returns (flow of level 1, [flow per level, coarsest first], minC of level 1); with runner_up=True also minC2 of level 1,
    the neighbour-guided runner-up cost of include/fsgm.h.  level_median=3 or 5: the median between levels of pyramidal_sgm."""
    return _one_shot(_bind_ng, "fsgm_ng_pyramid_params_default", "fsgm_pyramidal_sgm_ng", "pyramidal_sgm_ng", True, I0, I1, numPyd, device,
                     out, runner_up, level_median, overrides)


class FlowPPParams(C.Structure):
    _fields_ = [("matcher", C.c_int32), ("pyd", PyramidParams), ("ng", NgPyramidParams), ("speckle_max_diff", C.c_double),
                ("speckle_max_size", C.c_double), ("fb_thr", C.c_double), ("island_fraction", C.c_double), ("median", C.c_int32),
                ("device", C.c_int32)]


MATCHERS = {"pyd": 0, "ng": 1}
FLOW_PP_FIELDS = ("speckle_max_diff", "speckle_max_size", "fb_thr", "island_fraction")


def _bind_flow_pp(lib):
    if getattr(lib, "_flow_pp_bound", False):
        return
    vp, i32, prm = C.c_void_p, C.c_int32, C.POINTER(FlowPPParams)
    lib.fsgm_flow_pp_params_default.argtypes = [i32]
    lib.fsgm_flow_pp_params_default.restype = FlowPPParams
    lib.fsgm_pyramidal_flow_pp_host.argtypes = [i32, vp, vp, i32, i32, i32, prm, vp, vp, vp, vp, vp]
    lib.fsgm_pyramidal_flow_pp_device.argtypes = [i32, vp, vp, i32, i32, i32, prm, vp, vp, vp, vp, vp, vp, vp]
    lib.fsgm_pyramidal_flow_pp_time.argtypes = [i32, vp, vp, i32, i32, i32, prm, i32, i32, C.POINTER(C.c_float)]
    if hasattr(lib, "fsgm_pyramidal_flow_pp_host_u"):            # (an older build behind FSGM_LIB_PATH has neither)
        lib.fsgm_pyramidal_flow_pp_host_u.argtypes = [i32, vp, vp, i32, i32, i32, prm, i32, vp, vp, vp, vp, vp, vp]
        lib.fsgm_pyramidal_flow_pp_device_u.argtypes = [i32, vp, vp, i32, i32, i32, prm, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "fsgm_pyramidal_flow_pp_host_lm"):
        lib.fsgm_pyramidal_flow_pp_host_lm.argtypes = [i32, vp, vp, i32, i32, i32, prm, i32, i32, vp, vp, vp, vp, vp, vp]
        lib.fsgm_pyramidal_flow_pp_device_lm.argtypes = [i32, vp, vp, i32, i32, i32, prm, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib._flow_pp_bound = True


def flow_pp_params(lib, matcher, numPyd, device, median, overrides):
    """fsgm_flow_pp_params for `matcher` ("pyd" / "ng"): the chain's own fields and the matcher's overrides by name."""
    if matcher not in MATCHERS:
        raise ValueError(f"matcher must be 'pyd' or 'ng' (got {matcher!r})")
    _bind_flow_pp(lib)
    prm = lib.fsgm_flow_pp_params_default(MATCHERS[matcher])
    prm.device, prm.median = int(device), int(median)
    sub = prm.pyd if matcher == "pyd" else prm.ng
    if numPyd is not None:
        sub.numPyd = int(numPyd)
    for k, v in overrides.items():
        if k in FLOW_PP_FIELDS:
            setattr(prm, k, float(v))
        elif k not in ("numPyd", "device") and hasattr(sub, k):
            setattr(sub, k, int(v))
        else:
            raise TypeError(f"unknown pyramidal_flow_pp parameter {k!r} for matcher {matcher!r}")
    return prm


def _flow_pp_images(I0, I1, batch):
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    if I0.dtype != np.uint8 or I1.dtype != np.uint8 or I0.shape != I1.shape:
        raise TypeError("I0/I1 must be uint8 images of one shape")
    if batch is None:                                        # (3, H, W) is one RGB pair unless batch=True says three gray ones
        batch = I0.ndim == 4 or (I0.ndim == 3 and I0.shape[0] != 3)
    per = I0.ndim - (1 if batch else 0)
    if per not in (2, 3) or (per == 3 and I0.shape[-3] != 3):
        raise TypeError("images must be (height, width) or (3, height, width) per pair")
    if not batch:
        I0, I1 = I0[None], I1[None]
    return I0, I1, 1 if per == 2 else 3, batch


def uniqueness_ratio_of(ratio):
    """the ratio as the C ABI takes it: an integer in [0, 100]"""
    if isinstance(ratio, bool) or int(ratio) != ratio or not 0 <= int(ratio) <= 100:
        raise ValueError(f"uniqueness_ratio must be an integer in [0, 100] (got {ratio!r})")
    return int(ratio)


def pyramidal_flow_pp(I0, I1, numPyd=None, matcher="pyd", *, median=0, batch=None, device=0, uniqueness_ratio=None, level_median=0,
                      **overrides):
    """The consistency-checked, filtered flow of a pyramidal matcher (matcher="pyd": pyramidal_sgm, "ng": pyramidal_sgm_ng):
    forward and backward flow from one run of a plan of twice the batch, then on the device the chain of test.m:45-49 on
    vectors -- speckle filter of both flows, forward-backward check, island removal, KITTI hole fill, and vmf's median with
    median=1.  Images (height, width) or RGB (3, height, width) uint8, or a batch with a leading N (batch=None infers it).
    numPyd=None is the matcher's default.  Keyword overrides: speckle_max_diff (2), speckle_max_size (100), fb_thr (2.0),
    island_fraction (0.1) and the matcher's own parameters by name.

    Returns (flow_pp, flow_checked, flow_fwd, flow_bwd, minC): flow_pp (.., 3, height, width) float64 -- the filled u, v and
    the validity plane (1 where flow_checked is a number); flow_checked (.., 2, height, width) with NaN where rejected; the
    raw flows of both directions; minC (.., height, width) uint32 of the forward run.

    uniqueness_ratio=r (an integer in [0, 100]): the matcher also reports its runner-up cost, and the uniqueness test of
    fsgm_amd.uniqueness_filter blanks the ambiguous pixels of the forward and of the backward flow, each by its own costs, ahead
    of the chain.  The call then returns the five outputs plus minC2 of the forward run; the raw flows stay raw, and r = 0 gives
    the same five outputs as a call without the keyword.

    level_median=3 or 5: both directions run with the median between levels (pyramidal_sgm's keyword); flow_fwd and flow_bwd are
    the raw level-1 flows of those runs.  It combines with uniqueness_ratio."""
    level_median = level_median_of(level_median)
    lib = _lib.load()
    _bind(lib)
    _bind_ng(lib)
    I0, I1, ch, batched = _flow_pp_images(I0, I1, batch)
    N, H, W = I0.shape[0], I0.shape[-2], I0.shape[-1]
    prm = flow_pp_params(lib, matcher, numPyd, device, median, overrides)
    pp = np.empty((N, 3, H, W), np.float64)
    checked, fwd, bwd = (np.empty((N, 2, H, W), np.float64) for _ in range(3))
    minC = np.empty((N, H, W), np.uint32)
    minC2 = np.empty((N, H, W), np.uint32) if uniqueness_ratio is not None else None
    ratio = (uniqueness_ratio_of(uniqueness_ratio) if uniqueness_ratio is not None else 0,)
    fn, switches, second = _entry(lib, "fsgm_pyramidal_flow_pp_host", "_u", level_median, minC2, ratio)
    check(fn(N, ptr(I0), ptr(I1), W, H, ch, C.byref(prm), *switches, ptr(pp), ptr(checked), ptr(fwd), ptr(bwd), ptr(minC), *second))
    outs = (pp, checked, fwd, bwd, minC) + ((minC2,) if minC2 is not None else ())
    return outs if batched else tuple(o[0] for o in outs)


def pyramidal_flow_pp_time(I0, I1, numPyd=None, matcher="pyd", *, warmup=2, iters=10, batch=None, device=0, **overrides):
    """(ms of the batch-2N pyramid run, ms of the chain behind it), averages over `iters` runs by HIP events on the plan's stream."""
    lib = _lib.load()
    _bind(lib)
    _bind_ng(lib)
    I0, I1, ch, _ = _flow_pp_images(I0, I1, batch)
    N, H, W = I0.shape[0], I0.shape[-2], I0.shape[-1]
    prm = flow_pp_params(lib, matcher, numPyd, device, 0, overrides)
    ms = (C.c_float * 2)()
    check(lib.fsgm_pyramidal_flow_pp_time(N, ptr(I0), ptr(I1), W, H, ch, C.byref(prm), int(warmup), int(iters), ms))
    return float(ms[0]), float(ms[1])
