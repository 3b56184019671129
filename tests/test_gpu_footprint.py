"""Footprint of every device-pointer entry point: a call writes only its outputs and its results depend only on its inputs.

Each row of CASES names one C entry and a function that makes the ordinary call -- the entry on plain, separately allocated
tensors, through the package's own wrappers and binders -- and says which tensors were its inputs and outputs.  The call is
recorded (tests/footprint.py) and made again, through ctypes on torch's current stream, with every pointer swapped for a tensor
carved from an arena with guard bands, in two placements.  Per row and placement:
  1. same results     every output equals the ordinary call's (NaN positions equal, numbers equal)
  2. no stray write   every byte of the arena outside the outputs is unchanged (guards 0x00).  A stray store of zeros is invisible
                      against 0x00 guards, one of 0xFF bytes against the others: the check is made in both arenas and detection
                      relies on both patterns.  A stray store of an input's own value back into it is invisible to any arena.
  3. no stray read    the same call in a second arena of identical layout with guards 0xFF (NaN as a double, 255 as a cost, -1
                      as an int) gives bit-identical outputs, and again no stray write
  4. fully written    no poison (0xCD) is left in an output, PARTIAL below excepted
Assertion 3 sees a read of the caller's memory.  It is blind where a kernel reads past the end of the plan's own buffers: the
sgm(C), sgm2d(C), stereo, epipolar and pyramid WTAs read the plan's cost and path volumes (C is ingested into them; only bestD,
minC, minC2, mvSub, flow and S are bound to the caller's arrays), so their parabola's "next pixel's d = 0" read is outside what
an arena can show.  What it does see: the ingest kernels' loads of C, the cost kernels' image rows, the hint and guide reads and
every post stage's neighbour reads.
tests/test_footprint_table_cpu.py asserts that every fsgm_*_device* function of include/fsgm.h has a row here.

The per-frame pointer structs fsgm_epi_in / fsgm_epi_out hold one pointer per array for the whole contiguous batch (epi_run_device,
capi_epi.hip, checks n * H * W elements behind each): each such pointer gets one carved tensor.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import torch  # noqa: I001 -- before the library
from fsgm_amd import torch_ops, synth, EpiPlan, PydPlan  # noqa: E402
from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.sgm import last_kernel as sgm_kernel  # noqa: E402
from fsgm_amd.sgm2d import last_kernel as sgm2d_kernel  # noqa: E402
from tests import edge_inputs as E  # noqa: E402
from tests import footprint as F  # noqa: E402
from tests.footprint_table import DEVICE_ENTRIES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = torch_ops._L

# Outputs that include/fsgm.h documents as partly written: (entry, output) -> the header's words.  None so far: every output of
# every entry below is stated as a full array.
PARTIAL = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u32(*shape):
    return torch.empty(shape, dtype=torch.uint32, device=DEV)


def _f64(*shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def _status():
    return torch.empty((), dtype=torch.int32, device=DEV)


def _named(names, tensors):
    assert len(names) == len(tensors), (names, len(tensors))
    return dict(zip(names, tensors))


CASES = []           # (id, entry, fn); fn(ctx) makes the ordinary call and returns dict(inputs=, outputs=[, aliased=, opaque=, kernel=, probe=, reset=])


def case(entry, ident):
    def deco(fn):
        CASES.append(pytest.param(entry, fn, id=f"{entry}-{ident}"))
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ sgm(C)
def _volumes(W, H, D, n, seed, cmax, layout):
    v = np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])
    return _t(v if layout == "hwd" else v.transpose(0, 3, 1, 2))


def _sgm_case(entry, ident, W, H, D, n, layout, kernel, *, P=(7, 100), paths=4, bound=255, mode=0, adaptive=0, **kw):
    @case(entry, ident)
    def fn(ctx):
        Cv = _volumes(W, H, D, n, 3 + W + D, bound, layout)
        guide = _t(np.stack([synth.uniform_u8(5 + f, (H, W)) for f in range(n)])) if adaptive else None
        outs = torch_ops.sgm(Cv, *P, layout=layout, paths=paths, cost_bound=bound, agg_mode=mode, adaptive_p2=adaptive, guide=guide,
                             return_sum=True, return_status=True, **kw)
        names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("S", "status")
        ins = {"C": Cv, **({"guide": guide} if adaptive else {})}
        return dict(inputs=ins, outputs=_named(names, outs), kernel=(sgm_kernel, kernel))


_sgm_case("fsgm_sgm_device", "D16-hwd-packed", 37, 11, 16, 3, "hwd", "packed16/wrap")
_sgm_case("fsgm_sgm_device", "D48-dhw-12-a-lane", 65, 11, 48, 1, "dhw", "packed16/wrap", paths=8)
_sgm_case("fsgm_sgm_device", "D24-hwd-generic-one-row", 37, 1, 24, 3, "hwd", "generic")
_sgm_case("fsgm_sgm_device", "D300-dhw-generic-guide", 37, 11, 300, 1, "dhw", "generic", adaptive=1)
_sgm_case("fsgm_sgm_device", "D16-sweeps", 37, 11, 16, 3, "dhw", "sweep16/nowrap", P=(6, 32), paths=8, bound=24, mode=2)
_sgm_case("fsgm_sgm_device", "D128-band-sweeps-second-band", 17, 65, 128, 3, "dhw", "band16/nowrap", P=(6, 32), paths=8, bound=24, mode=4)
_sgm_case("fsgm_sgm_device_ru", "D16-dhw", 65, 11, 16, 3, "dhw", "packed16/wrap", runner_up=True)
_sgm_case("fsgm_sgm_device_ru", "D48-hwd-one-column", 1, 11, 48, 3, "hwd", "packed16/wrap", runner_up=True)
_sgm_case("fsgm_sgm_device_ru", "D300-hwd", 37, 11, 300, 1, "hwd", "generic", runner_up=True, paths=8)
_sgm_case("fsgm_sgm_device_ru", "D24-dhw", 65, 1, 24, 1, "dhw", "generic", runner_up=True)
_sgm_case("fsgm_sgm_device_exact", "D16-hwd", 37, 11, 16, 3, "hwd", "packed16/exact", arith="exact", paths=8)
_sgm_case("fsgm_sgm_device_exact", "D48-dhw", 65, 11, 48, 1, "dhw", "packed16/exact", arith="exact")
_sgm_case("fsgm_sgm_device_exact", "D24-dhw", 37, 11, 24, 3, "dhw", "generic/exact", arith="exact")
_sgm_case("fsgm_sgm_device_exact", "D300-hwd-guide", 65, 1, 300, 1, "hwd", "generic/exact", arith="exact", adaptive=1)


def _ingest_case(entry, ident, make_plan, D, layout):
    @case(entry, ident)
    def fn(ctx):
        plan = ctx.enter_context(make_plan())
        n, H, W = plan.batch, plan.H, plan.W
        Cv = _volumes(W, H, D, n, 9, 255, "hwd" if layout == "hwd" else "dhw")
        zero = torch.zeros_like(Cv)
        status = plan.ingest_cost(Cv, layout=layout, cost_bound=255, return_status=True)

        def probe():
            torch.cuda.synchronize()
            return np.stack([plan.download_cost(f) for f in range(n)])

        def reset():                                              # the plan's volumes hold something else before each replay
            plan.ingest_cost(zero, layout=layout, cost_bound=255, check=True)
            assert not probe().any()
        return dict(inputs={"C": Cv}, outputs={"status": status}, opaque=[plan._h.value], probe=probe, reset=reset)


_ingest_case("fsgm_epi_plan_ingest_cost_device", "D48-dhw", lambda: EpiPlan(37, 11, 48, 3, vz_to_disp=0), 48, "dhw")
_ingest_case("fsgm_epi_plan_ingest_cost_device", "D17-hwd", lambda: EpiPlan(65, 1, 17, 1, vz_to_disp=0), 17, "hwd")
_ingest_case("fsgm_pyd_plan_ingest_cost_device", "3x5-dhw_yx", lambda: PydPlan(37, 11, 37, 11, 1, 2, 0, batch=3), 15, "dhw_yx")
_ingest_case("fsgm_pyd_plan_ingest_cost_device", "13x9-hwd", lambda: PydPlan(65, 1, 65, 1, 6, 4, 0, batch=1), 117, "hwd")


# ------------------------------------------------------------------------------------------------ sgm2d(C)
@functools.lru_cache(maxsize=None)
def _rows_available():
    """whether this device's plans hold the row-packed kernels (tests/test_gpu_sgm2d.py::rows_available); asked before the
    ordinary call, since it is itself a call that fsgm_sgm2d_last_kernel then names"""
    from fsgm_amd import sgm2d_batch
    sgm2d_batch(np.zeros((9, 2, 3), np.uint8), 1, 1, 6, 32, layout="dhw", cost_bound=24)
    return sgm2d_kernel().startswith("rows")


def _sgm2d_case(entry, ident, W, H, rX, rY, n, layout, kernel, *, bound=24, hints=True, adaptive=0, **kw):
    @case(entry, ident)
    def fn(ctx):
        assert _rows_available(), "this device's plans hold no row-packed kernels: the rows and rows/wide rows cannot run"
        Sx, Sy = 2 * rX + 1, 2 * rY + 1
        v = np.stack([synth.cost_volume(W, H, Sx * Sy, 3 + rX + 13 * f, bound) for f in range(n)])
        v[-1, -1, -1, -1] = bound
        Cv = _t(v if layout == "hwd" else v.transpose(0, 3, 1, 2))
        hm = _t(np.stack([synth.hint_map(W + 3, H + 3, "general", seed=40 + 5 * f, amp=3.0) for f in range(n)])) if hints else None
        guide = _t(np.stack([synth.uniform_u8(5 + f, (H, W)) for f in range(n)])) if adaptive else None
        outs = torch_ops.sgm2d(Cv, rX, rY, 6, 32, layout=layout, hints=hm, guide=guide, cost_bound=bound, adaptive_p2=adaptive,
                               return_flow=True, return_sum=True, return_status=True, **kw)
        names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("mvSub", "flow", "S", "status")
        ins = {"C": Cv, **({"preMv": hm} if hints else {}), **({"guide": guide} if adaptive else {})}
        return dict(inputs=ins, outputs=_named(names, outs), kernel=(sgm2d_kernel, kernel))


_sgm2d_case("fsgm_sgm2d_device", "rows-3x5-hints", 37, 11, 1, 2, 3, "dhw", "rows")
_sgm2d_case("fsgm_sgm2d_device", "generic-13x9-guide", 65, 11, 6, 4, 1, "hwd", "generic", hints=False, adaptive=1)
_sgm2d_case("fsgm_sgm2d_device", "generic-wrap-one-row", 37, 1, 2, 1, 3, "dhw_yx", "generic/wrap", bound=255)
_sgm2d_case("fsgm_sgm2d_device_ru", "rows-wide-5x3-hints", 65, 11, 2, 1, 1, "dhw_yx", "rows/wide", runner_up=True)
_sgm2d_case("fsgm_sgm2d_device_ru", "generic-wrap-guide", 37, 11, 1, 2, 3, "hwd", "generic/wrap", bound=255, adaptive=1, runner_up=True)
_sgm2d_case("fsgm_sgm2d_device_ru", "rows-one-column", 1, 11, 1, 2, 3, "dhw", "rows", runner_up=True)
_sgm2d_case("fsgm_sgm2d_device_exact", "exact-hints-guide-ru", 37, 11, 1, 2, 3, "dhw", "generic/exact", adaptive=1, runner_up=True,
            arith="exact")
_sgm2d_case("fsgm_sgm2d_device_exact", "exact-13x9", 65, 1, 6, 4, 1, "hwd", "generic/exact", bound=255, hints=False, arith="exact")


# ------------------------------------------------------------------------------------------------ rectified stereo
def _stereo_pair(W, H, n, D):
    pairs = [synth.image_pair(W, H, D, seed=3 + f) for f in range(n)]
    return _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))


def _stereo_case(entry, ident, W, H, n, *, fb=0, **kw):
    @case(entry, ident)
    def fn(ctx):
        left, right = _stereo_pair(W, H, n, 16)
        outs = torch_ops.stereo_sgm(left, right, 16, 6, 64, fb_check=fb, return_status=True, **kw)
        names = ("disp", "minC") + (("conf", "disp2") if fb else ()) + (("minC2",) if kw.get("runner_up") else ()) + ("status",)
        return dict(inputs={"I1": left, "I2": right}, outputs=_named(names, outs))


for _W, _H, _n in ((255, 11, 3), (257, 1, 1)):
    _stereo_case("fsgm_stereo_sgm_device_opts", f"W{_W}", _W, _H, _n, fb=_n == 3, adaptive_p2=int(_n == 1))
    _stereo_case("fsgm_stereo_sgm_device_range", f"W{_W}", _W, _H, _n, fb=_n == 1, d_min=-4, paths=8)
    _stereo_case("fsgm_stereo_sgm_device_ru", f"W{_W}", _W, _H, _n, fb=_n == 3, d_min=3, runner_up=True)


def _stereo_plain_case(W, H, n, fb):
    @case("fsgm_stereo_sgm_device", f"W{W}")
    def fn(ctx):
        left, right = _stereo_pair(W, H, n, 16)
        disp, minC, disp2, status = _u32(n, H, W), _u32(n, H, W), _u32(n, H, W), _status()
        conf = torch.empty((n, H, W), dtype=torch.uint8, device=DEV)
        prm = torch_ops._stereo_params(4, 1, -1, fb, 0)
        _lib.check(L.fsgm_stereo_sgm_device(n, _p(left), _p(right), W, H, 16, 6, 64, C.byref(prm), _p(disp), _p(minC),
                                            _p(conf) if fb else None, _p(disp2) if fb else None, _stream(), _p(status)))
        outs = {"disp": disp, "minC": minC, **({"conf": conf, "disp2": disp2} if fb else {}), "status": status}
        return dict(inputs={"I1": left, "I2": right}, outputs=outs)


_stereo_plain_case(255, 1, 1, 1)
_stereo_plain_case(257, 11, 3, 0)


def _stereo_pp_case(W, H, n, in_fill):
    @case("fsgm_stereo_sgm_pp_device", f"W{W}")
    def fn(ctx):
        left, right = _stereo_pair(W, H, n, 16)
        outs = torch_ops.stereo_sgm_pp(left, right, 16, 6, 64, in_fill=in_fill, return_status=True)
        return dict(inputs={"I1": left, "I2": right}, outputs=_named(("disp_pp", "disp_checked", "disp", "minC", "disp2", "status"), outs))


_stereo_pp_case(255, 11, 3, 1)
_stereo_pp_case(257, 11, 1, 0)


def _disparities(W, H, n, seed):
    """f64 disparity maps on the 1/256 grid with NaN holes, as the matcher and the chain produce them"""
    r = E.rng(seed)
    d = np.round(r.rand(n, H, W) * 12 * 256) / 256
    d[r.rand(n, H, W) < 0.1] = np.nan
    return d


def _stereo_fb_case(W, H, n, fused):
    @case("fsgm_stereo_fb_check_device", f"W{W}-{'fused' if fused else 'two-maps'}")
    def fn(ctx):
        D1 = _t(_disparities(W, H, n, 5))
        if fused:
            out, second, status = torch_ops.stereo_fb_check(D1, None, 0, -1, 2.0, return_second=True, return_status=True)
            return dict(inputs={"D1": D1}, outputs={"D1checked": out, "D2out": second, "status": status})
        D2 = _t(_disparities(W, H, n, 6))
        out, status = torch_ops.stereo_fb_check(D1, D2, 0, -1, 2.0, return_status=True)
        return dict(inputs={"D1": D1, "D2": D2}, outputs={"D1checked": out, "status": status})


_stereo_fb_case(255, 11, 3, True)
_stereo_fb_case(257, 1, 1, False)
_stereo_fb_case(257, 11, 3, True)


def _disp_from_first_case(W, H, n):
    @case("fsgm_stereo_disp_from_first_device", f"W{W}")
    def fn(ctx):
        D1, D2, status = _t(_disparities(W, H, n, 7)), _f64(n, H, W), _status()
        _lib.check(L.fsgm_stereo_disp_from_first_device(n, _p(D1), W, H, 0, -1, _p(D2), 0, _stream(), _p(status)))
        return dict(inputs={"D1": D1}, outputs={"D2": D2, "status": status})


_disp_from_first_case(255, 11, 3)
_disp_from_first_case(257, 1, 1)


# ------------------------------------------------------------------------------------------------ epipolar
def _epi_inputs(W, H, n, D):
    pairs = [synth.image_pair(W, H, D, seed=1 + f) for f in range(n)]
    pd0, nd, off = synth.epi_maps(W, H, "general")
    rep = lambda a: _t(np.stack([a] * n))  # noqa: E731
    return _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs])), rep(pd0), rep(nd), rep(off)


def _epi_opts_case(entry, W, H, n, fb, adaptive, paths):
    linear = "linear" in entry

    @case(entry, f"{W}x{H}x{n}")
    def fn(ctx):
        I1, I2, pd0, nd, off = _epi_inputs(W, H, n, 16)
        kw = dict(paths=paths, fb_check=fb, adaptive_p2=adaptive, return_status=True)
        outs = (torch_ops.calc_cost_sgm_linear(I1, I2, 16, pd0, nd, 6, 64, **kw) if linear
                else torch_ops.calc_cost_sgm(I1, I2, 16, 0.3, pd0, nd, off, 6, 64, **kw))
        names = ("bestD", "minC") + (("conf", "bestD2") if fb else ()) + ("status",)
        ins = {"I1": I1, "I2": I2, "pixelPosD0": pd0, "normDir": nd, **({} if linear else {"offset": off})}
        return dict(inputs=ins, outputs=_named(names, outs))


_epi_opts_case("fsgm_calc_cost_sgm_device_opts", 37, 11, 3, 1, 0, 8)
_epi_opts_case("fsgm_calc_cost_sgm_device_opts", 65, 11, 1, 0, 1, 4)
_epi_opts_case("fsgm_calc_cost_sgm_linear_device_opts", 65, 11, 3, 0, 1, 8)
_epi_opts_case("fsgm_calc_cost_sgm_linear_device_opts", 37, 11, 1, 1, 0, 4)


def _epi_plain_case(entry, W, H, n, fb):
    linear = "linear" in entry

    @case(entry, f"{W}x{H}x{n}")
    def fn(ctx):
        I1, I2, pd0, nd, off = _epi_inputs(W, H, n, 16)
        bestD, minC, bestD2, status = _u32(n, H, W), _u32(n, H, W), _u32(n, H, W), _status()
        conf = torch.empty((n, H, W), dtype=torch.uint8, device=DEV)
        e, o = torch_ops._epi_structs(I1, I2, pd0, nd, None if linear else off, W, H, 16, 0.0 if linear else 0.3, 6, 64, bestD, minC,
                                      conf if fb else None, bestD2 if fb else None)
        prm = torch_ops._epi_params(4, 1, 0 if linear else 1, 0, fb)
        _lib.check(getattr(L, entry)(n, C.byref(e), C.byref(o), C.byref(prm), _stream(), _p(status)))
        ins = {"I1": I1, "I2": I2, "pixelPosD0": pd0, "normDir": nd, **({} if linear else {"offset": off})}
        outs = {"bestD": bestD, "minC": minC, **({"conf": conf, "bestD2": bestD2} if fb else {}), "status": status}
        return dict(inputs=ins, outputs=outs)


_epi_plain_case("fsgm_calc_cost_sgm_device", 37, 11, 3, 0)
_epi_plain_case("fsgm_calc_cost_sgm_device", 65, 11, 1, 1)
_epi_plain_case("fsgm_calc_cost_sgm_linear_device", 65, 11, 3, 1)
_epi_plain_case("fsgm_calc_cost_sgm_linear_device", 37, 11, 1, 0)


def _plan_run_case(W, H, D, n, mode, paths, kernel):
    @case("fsgm_epi_plan_run_device", f"{W}x{H}x{n}-mode{mode}")
    def fn(ctx):
        I1, I2, pd0, nd, off = _epi_inputs(W, H, n, D)
        plan = ctx.enter_context(EpiPlan(W, H, D, n, paths=paths))
        plan.set_penalties(6, 64, 0.3)
        plan.set_agg_mode(mode)
        outs = plan.run_tensors(I1, I2, pd0, nd, off, return_status=True)
        ins = {"I1": I1, "I2": I2, "pixelPosD0": pd0, "normDir": nd, "offset": off}
        return dict(inputs=ins, outputs=_named(("bestD", "minC", "status"), outs), opaque=[plan._h.value],
                    kernel=((lambda: plan.kernel_name), kernel))


_plan_run_case(37, 11, 16, 3, 1, 4, "packed16/nowrap")
_plan_run_case(65, 11, 16, 3, 4, 8, "band16/nowrap")


def _geometries(W, H, n):
    kinds = ("forward", "contract", "forward")
    g = [synth.epi_geometry(W, H, kinds[f]) for f in range(n)]
    return [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], [x[3] for x in g]


def _epipolar_case(entry, W, H, n, rgb):
    @case(entry, f"{W}x{H}x{n}{'-rgb' if rgb else ''}")
    def fn(ctx):
        pairs = [synth.image_pair(W, H, 16, seed=21 + f) for f in range(n)]
        stack = lambda k: _t(np.stack([np.stack([p[k]] * 3) if rgb else p[k] for p in pairs]))  # noqa: E731
        I0, I1 = stack(0), stack(1)
        if entry == "fsgm_epipolar_sgm_of_device":
            outs, names = torch_ops.epipolar_sgm_of(I0, I1, *_geometries(W, H, n), 16, 0.3, return_status=True), ("flow", "minC", "status")
        else:
            outs = torch_ops.epipolar_flow_pp(I0, I1, *_geometries(W, H, n), 16, 0.3, paths=8, return_status=True)
            names = ("flow", "flow2", "D1", "minC", "status")
        return dict(inputs={"I0": I0, "I1": I1}, outputs=_named(names, outs))


_epipolar_case("fsgm_epipolar_sgm_of_device", 37, 11, 3, False)
_epipolar_case("fsgm_epipolar_sgm_of_device", 65, 11, 1, True)
_epipolar_case("fsgm_epipolar_flow_pp_device", 65, 11, 3, True)
_epipolar_case("fsgm_epipolar_flow_pp_device", 37, 11, 1, False)


def _epi_postprocess_case(W, H, n, seed):
    @case("fsgm_epi_postprocess_device", f"{W}x{H}x{n}")
    def fn(ctx):
        r = E.rng(seed)
        D1 = _t(E.post_maps(r, W, H, n, 5.0, 0.3, 17.0))
        Pd0, nd, O = (_t(a) for a in E.post_geometry(r, W, H, n))
        outs = torch_ops.epi_postprocess(D1, Pd0, nd, O, 0.3, 17.0, 16.0, return_status=True)
        return dict(inputs={"D1": D1, "Pd0": Pd0, "normDirect": nd, "O": O}, outputs=_named(("filterD1", "filterD2", "disp", "status"), outs))


_epi_postprocess_case(37, 11, 3, 31)
_epi_postprocess_case(65, 1, 1, 32)
_epi_postprocess_case(1, 11, 3, 33)


# ------------------------------------------------------------------------------------------------ pyramids
def _pyramid_pairs(W, H, n, ch):
    pairs = [E.image_pair(E.rng(11 + k), W, H, ch, seed=11 + k) for k in range(n)]
    return _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))


def _pyramid_case(entry, W, H, n, ch, **kw):
    op = torch_ops.pyramidal_sgm_ng if "_ng_" in entry else torch_ops.pyramidal_sgm

    @case(entry, f"{W}x{H}x{n}" + "".join(f"-{k}{int(v)}" for k, v in kw.items()))
    def fn(ctx):
        I0, I1 = _pyramid_pairs(W, H, n, ch)
        outs = op(I0, I1, 3, batch=True, return_status=True, **kw)
        names = ("flow", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("status",)
        return dict(inputs={"I0": I0, "I1": I1}, outputs=_named(names, outs))


for _ng in ("", "_ng"):
    _pyramid_case(f"fsgm_pyramidal_sgm{_ng}_device", 61, 47, 1, 3)
    _pyramid_case(f"fsgm_pyramidal_sgm{_ng}_device", 37, 23, 3, 1)
    _pyramid_case(f"fsgm_pyramidal_sgm{_ng}_device_ru", 37, 23, 3, 1, runner_up=True)
    _pyramid_case(f"fsgm_pyramidal_sgm{_ng}_device_lm", 61, 47, 1, 1, level_median=3, runner_up=True)
    _pyramid_case(f"fsgm_pyramidal_sgm{_ng}_device_lm", 37, 23, 3, 3, level_median=5)


def _flow_pp_case(entry, W, H, n, matcher, **kw):
    @case(entry, f"{matcher}-{W}x{H}x{n}" + "".join(f"-{k}{int(v)}" for k, v in kw.items()))
    def fn(ctx):
        I0, I1 = _pyramid_pairs(W, H, n, 1)
        outs = torch_ops.pyramidal_flow_pp(I0, I1, 3, matcher, batch=True, return_status=True, **kw)
        names = ("flow_pp", "flow_checked", "flow_fwd", "flow_bwd", "minC") + (("minC2",) if "uniqueness_ratio" in kw else ()) + ("status",)
        return dict(inputs={"I0": I0, "I1": I1}, outputs=_named(names, outs))


_flow_pp_case("fsgm_pyramidal_flow_pp_device", 37, 23, 3, "pyd")
_flow_pp_case("fsgm_pyramidal_flow_pp_device", 61, 47, 1, "ng", median=1)
_flow_pp_case("fsgm_pyramidal_flow_pp_device_u", 37, 23, 3, "ng", uniqueness_ratio=15)
_flow_pp_case("fsgm_pyramidal_flow_pp_device_u", 61, 47, 1, "pyd", uniqueness_ratio=15)
_flow_pp_case("fsgm_pyramidal_flow_pp_device_lm", 37, 23, 3, "pyd", level_median=3, uniqueness_ratio=15)
_flow_pp_case("fsgm_pyramidal_flow_pp_device_lm", 61, 47, 1, "ng", level_median=5)


# ------------------------------------------------------------------------------------------------ post stages
POST_SHAPES = ((37, 11, 3), (65, 1, 1), (1, 11, 3))


def _flow_stage_case(entry, W, H, n, ch, call):
    @case(entry, f"{W}x{H}x{n}x{ch}")
    def fn(ctx):
        flow = _t(E.vmf_flows(E.rng(50 + W + ch), W, H, n, ch))
        out = call(flow, W, H, n, ch)
        return dict(inputs={"flow": flow}, outputs={"out": out})


def _raw(entry, *mid):
    def call(flow, W, H, n, ch):
        out = torch.empty_like(flow)
        _lib.check(getattr(L, entry)(n, _p(flow), W, H, *mid, _p(out), 0, _stream()))
        return out
    return call


for _i, (_W, _H, _n) in enumerate(POST_SHAPES):
    _flow_stage_case("fsgm_vmf_device", _W, _H, _n, _i + 1, lambda flow, W, H, n, ch: torch_ops.vmf(flow))
    _flow_stage_case("fsgm_flow_speckle_filter_device", _W, _H, _n, 2, _raw("fsgm_flow_speckle_filter_device", 2.0, 5.0))
    _flow_stage_case("fsgm_flow_in_fill_device", _W, _H, _n, 2, _raw("fsgm_flow_in_fill_device"))
    _flow_stage_case("fsgm_flow_level_hints_device", _W, _H, _n, 2, lambda flow, W, H, n, ch, s=(3, 5, 3)[_i]: torch_ops.flow_level_hints(flow, s))


def _flow_fb_case(W, H, n):
    @case("fsgm_flow_fb_check_device", f"{W}x{H}x{n}")
    def fn(ctx):
        f, b = _t(E.vmf_flows(E.rng(60 + W), W, H, n, 2)), _t(E.vmf_flows(E.rng(61 + W), W, H, n, 2))
        return dict(inputs={"f": f, "b": b}, outputs={"fChecked": torch_ops.flow_fb_check(f, b, 2.0)})


def _uniqueness_inputs(W, H, n, planes, seed):
    r = E.rng(seed)
    m = E.vmf_flows(r, W, H, n, planes)
    minC = r.randint(0, 2000, (n, H, W)).astype(np.uint32)
    minC2 = (minC * r.choice([1.0, 1.1, 1.2, 3.0], (n, H, W))).astype(np.uint32)
    minC2[r.rand(n, H, W) < 0.1] = 0xFFFFFFFF
    return _t(m if planes == 2 else m[:, 0]), _t(minC), _t(minC2)


def _uniqueness_case(W, H, n, planes, alias):
    entry = "fsgm_uniqueness_filter_planes_device" if planes else "fsgm_uniqueness_filter_device"

    @case(entry, f"{W}x{H}x{n}" + (f"-planes{planes}" if planes else "") + ("-out-is-map" if alias else ""))
    def fn(ctx):
        m, minC, minC2 = _uniqueness_inputs(W, H, n, planes or 1, 70 + W)
        ins = {"minC": minC, "minC2": minC2}
        if not alias:
            op = torch.ops.fsgm.uniqueness_filter_planes if planes else torch.ops.fsgm.uniqueness_filter
            out, status = op(m, minC, minC2, 15, *((planes,) if planes else ()))
            return dict(inputs={"map": m, **ins}, outputs={"out": out, "status": status})
        before, status = m.clone(), _status()                     # the documented aliasing: out may be map itself
        _lib.check(getattr(L, entry)(n, _p(m), _p(minC), _p(minC2), W, H, *((planes,) if planes else ()), 15, _p(m), 0, _stream(), _p(status)))
        return dict(inputs=ins, aliased={"map=out": (m, before)}, outputs={"status": status})


for _W, _H, _n in POST_SHAPES:
    _flow_fb_case(_W, _H, _n)
    _uniqueness_case(_W, _H, _n, 0, False)
    _uniqueness_case(_W, _H, _n, 2 if _n == 3 else 1, False)
_uniqueness_case(37, 11, 3, 0, True)
_uniqueness_case(65, 1, 1, 2, True)

ENTRIES = sorted({p.values[0] for p in CASES})
assert ENTRIES == sorted(DEVICE_ENTRIES), (set(ENTRIES) ^ set(DEVICE_ENTRIES), "rows and tests/footprint_table.py differ")


# ------------------------------------------------------------------------------------------------ the check
def _specs(info, args):
    """(name, role, ordinary tensor, initial content) of every tensor of the call, in the order the C arguments name them; every
    pointer among the arguments must be one of them, the stream or a handle the case declares"""
    known = {}
    for role in ("inputs", "outputs", "aliased"):
        for name, t in info.get(role, {}).items():
            t, init = t if role == "aliased" else (t, t)
            assert t.numel() > 0 and t.is_contiguous(), name
            assert t.data_ptr() not in known, f"{name} shares its address with {known.get(t.data_ptr())}"
            known[t.data_ptr()] = (name, {"inputs": "in", "outputs": "out", "aliased": "inout"}[role], t, init)
    opaque = set(info.get("opaque", ())) | {torch.cuda.current_stream().cuda_stream}
    seen = []
    for ptr in F.pointers_of(args):
        if ptr in known:
            if ptr not in seen:
                seen.append(ptr)
        else:
            assert ptr in opaque, f"the call got a pointer {ptr:#x} that the case does not name"
    missing = [known[p][0] for p in known if p not in seen]
    assert not missing, f"the case names tensors the call never got: {missing}"
    return [known[p] for p in seen]


@pytest.mark.parametrize("placement", F.PLACEMENTS)
@pytest.mark.parametrize("entry,fn", CASES)
def test_footprint(gpu_lib, entry, fn, placement):
    with contextlib.ExitStack() as ctx:
        info, args, real = F.record(L, entry, lambda: fn(ctx))
        torch.cuda.synchronize()
        specs = _specs(info, args)
        want = {name: t.clone() for name, role, t, _ in specs if role != "in"}
        if "status" in want:
            assert int(want["status"].item()) == 0
        getter, kernel = info.get("kernel", (None, None))
        assert getter is None or getter() == kernel, f"the ordinary call ran {getter()!r}, the row is about {kernel!r}"
        probe = info.get("probe")
        state = probe() if probe else None
        first = None
        for pattern in (0x00, 0xFF):
            arena = F.Arena([(name, role, init) for name, role, _, init in specs], placement, pattern, DEV)
            swap = {t.data_ptr(): arena[name].data_ptr() for name, _, t, _ in specs}
            if "reset" in info:
                info["reset"]()
            _lib.check(F.replay(real, args, swap))
            torch.cuda.synchronize()
            assert getter is None or getter() == kernel
            got = arena.outputs()
            arena.check(pattern)                                  # 2. (and again under 3.); first: a stray write may also spoil a result
            for name, role, _, _ in specs:
                if role == "out" and (entry, name) not in PARTIAL:
                    arena.all_written(name)                       # 4. (before 1.: a missing write is named as such, not as a wrong value)
            for name, w in want.items():
                if first is None:
                    assert F.same(got[name], w), f"1. {name} differs from the ordinary call's ({placement})"
                else:
                    assert F.bit_identical(got[name], first[name]), f"3. {name} depends on memory outside the inputs ({placement})"
            if probe:
                np.testing.assert_array_equal(probe(), state)
            if first is None:
                first = {name: t.clone() for name, t in got.items()}


# ------------------------------------------------------------------------------------------------ host forms, one per family
# Each entry as include/fsgm.h spells it, inputs and outputs numpy arrays passed with _lib.ptr: once on plain arrays, then with every
# output carved from a guarded numpy array (tests/footprint.py, HostArena), guards 0x00 and again 0xFF.  Assertions 1 and 2.
from fsgm_amd import pyramid as _pyramid  # noqa: E402
import importlib  # noqa: E402

_sgm, _sgm2d, _epi = (importlib.import_module("fsgm_amd." + m) for m in ("sgm", "sgm2d", "epi"))    # (fsgm_amd.sgm the name is the function)
from fsgm_amd._lib import EpiIn, EpiOut, ptr  # noqa: E402

HOST_CASES = {}


def host_case(fn):
    HOST_CASES["fsgm_" + fn.__name__] = fn
    return fn


def _np_volumes(W, H, D, n, seed, cmax):
    return np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])


@host_case
def sgm_batch_host(lib, out):
    n, H, W, D = 3, 11, 37, 48
    Cv = _np_volumes(W, H, D, n, 3, 255)
    prm = _sgm.params(_sgm._bind(lib), paths=8, device=0, agg_mode=0, layout="hwd", cost_bound=255, adaptive_p2=0)
    return lib.fsgm_sgm_batch_host(n, ptr(Cv), W, H, D, 7, 100, C.byref(prm), None, ptr(out("bestD", (n, H, W), np.uint32)),
                                   ptr(out("minC", (n, H, W), np.uint32)), ptr(out("S", (n, H, W, D), np.uint32)))


@host_case
def sgm2d_batch_host(lib, out):
    n, H, W, rX, rY = 3, 11, 37, 1, 2
    Cv = _np_volumes(W, H, 15, n, 4, 24)
    hints = np.stack([synth.hint_map(W + 3, H + 3, "general", seed=40 + 5 * f, amp=3.0) for f in range(n)])
    _sgm2d._bind(lib)
    prm = _sgm2d.params(lib, device=0, layout="hwd", cost_bound=24)
    return lib.fsgm_sgm2d_batch_host(n, ptr(Cv), W, H, rX, rY, 6, 32, C.byref(prm), ptr(hints), W + 3, H + 3, None,
                                     ptr(out("bestD", (n, H, W), np.uint32)), ptr(out("minC", (n, H, W), np.uint32)),
                                     ptr(out("mvSub", (n, 2, H, W), np.float64)), ptr(out("flow", (n, 2, H, W), np.float64)),
                                     ptr(out("S", (n, H, W, 15), np.uint32)))


@host_case
def stereo_sgm_host_ru(lib, out):
    n, H, W = 3, 11, 255
    pairs = [synth.image_pair(W, H, 16, seed=3 + f) for f in range(n)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    prm, opt = _epi._stereo_params(4, 1, -1, 1, 0), _lib.options(0)
    return lib.fsgm_stereo_sgm_host_ru(n, ptr(left), ptr(right), W, H, 16, 6, 64, C.byref(prm), C.byref(opt), 3,
                                       ptr(out("disp", (n, H, W), np.int32)), ptr(out("minC", (n, H, W), np.uint32)),
                                       ptr(out("minC2", (n, H, W), np.uint32)), ptr(out("conf", (n, H, W), np.uint8)),
                                       ptr(out("disp2", (n, H, W), np.int32)))


@host_case
def calc_cost_sgm_batch_host(lib, out):
    """one carved array per frame and pointer: fsgm_epi_in / fsgm_epi_out are per-frame here"""
    n, H, W, D = 3, 11, 37, 16
    pd0, nd, off = synth.epi_maps(W, H, "general")
    ins, outs, keep = (EpiIn * n)(), (EpiOut * n)(), []
    for f in range(n):
        I1, I2 = synth.image_pair(W, H, D, seed=1 + f)
        keep.append((I1, I2))
        e, o = ins[f], outs[f]
        e.I1, e.I2, e.width, e.height, e.dMax, e.vMax = ptr(I1), ptr(I2), W, H, D, 0.3
        e.pixelPosD0, e.normDir, e.offset, e.P1, e.P2 = ptr(pd0), ptr(nd), ptr(off), 6, 64
        o.bestD, o.minC = ptr(out(f"bestD{f}", (H, W), np.uint32)), ptr(out(f"minC{f}", (H, W), np.uint32))
        o.conf, o.bestD2 = ptr(out(f"conf{f}", (H, W), np.uint8)), ptr(out(f"bestD2{f}", (H, W), np.uint32))
    prm = _epi._params(8, 1, 1, 0, 1)
    return lib.fsgm_calc_cost_sgm_batch_host(n, ins, outs, C.byref(prm))


def _pyramid_host(lib, out, entry, default, bind):
    W, H, numPyd = 37, 23, 3
    bind(lib)
    I0, I1 = E.image_pair(E.rng(11), W, H, 1, seed=11)
    prm = getattr(lib, default)()
    prm.numPyd, prm.device = numPyd, 0
    levels = [out(f"level{k}", (2, h, w), np.float64) for k, (w, h) in enumerate(_pyramid._level_sizes(W, H, numPyd))]
    ptrs = (C.c_void_p * len(levels))(*[a.ctypes.data for a in levels])
    return getattr(lib, entry)(ptr(I0), ptr(I1), W, H, 1, C.byref(prm), 3, ptr(out("flow", (2, H, W), np.float64)),
                               ptr(out("minC", (H, W), np.uint32)), ptr(out("minC2", (H, W), np.uint32)), ptrs)


@host_case
def pyramidal_sgm_host_lm(lib, out):
    return _pyramid_host(lib, out, "fsgm_pyramidal_sgm_host_lm", "fsgm_pyramid_params_default", _pyramid._bind)


@host_case
def pyramidal_sgm_ng_host_lm(lib, out):
    return _pyramid_host(lib, out, "fsgm_pyramidal_sgm_ng_host_lm", "fsgm_ng_pyramid_params_default", _pyramid._bind_ng)


@host_case
def pyramidal_flow_pp_host_lm(lib, out):
    n, W, H = 3, 37, 23
    _pyramid._bind_flow_pp(lib)
    pairs = [E.image_pair(E.rng(11 + k), W, H, 1, seed=11 + k) for k in range(n)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    prm = _pyramid.flow_pp_params(lib, "pyd", 3, 0, 0, {})
    flows = [ptr(out(name, (n, 2, H, W), np.float64)) for name in ("flow_checked", "flow_fwd", "flow_bwd")]
    return lib.fsgm_pyramidal_flow_pp_host_lm(n, ptr(I0), ptr(I1), W, H, 1, C.byref(prm), 15, 3, ptr(out("flow_pp", (n, 3, H, W), np.float64)),
                                              *flows, ptr(out("minC", (n, H, W), np.uint32)), ptr(out("minC2", (n, H, W), np.uint32)))


@host_case
def vmf_host(lib, out):
    W, H, ch = 37, 11, 3
    flow = E.vmf_flows(E.rng(53), W, H, 1, ch)[0]
    torch_ops._bind_post(lib)
    return lib.fsgm_vmf_host(ptr(flow), W, H, ch, ptr(out("flowMed", (ch, H, W), np.float64)), 0)


def _same_np(a, b):
    if a.dtype.kind == "f":
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("entry", sorted(HOST_CASES))
def test_host_footprint(gpu_lib, entry):
    plain, shapes = {}, []

    def alloc(name, shape, dtype):
        shapes.append((name, shape, dtype))
        plain[name] = np.full(shape, F.POISON, np.uint8).astype(dtype) if np.dtype(dtype).itemsize == 1 else \
            np.frombuffer(bytes([F.POISON]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
        return plain[name]

    _lib.check(HOST_CASES[entry](L, alloc))
    for pattern in (0x00, 0xFF):
        arena = F.HostArena(shapes, pattern)
        handed = []

        def carve(name, shape, dtype):
            handed.append(name)
            assert arena.views[name].shape == tuple(shape) and arena.views[name].dtype == np.dtype(dtype)
            return arena.views[name]

        _lib.check(HOST_CASES[entry](L, carve))
        assert handed == [s[0] for s in shapes]
        arena.check()                                             # 2.
        for name, want in plain.items():
            assert _same_np(arena.views[name], want), f"1. {name} differs from the call on plain arrays (guards {pattern:#04x})"
