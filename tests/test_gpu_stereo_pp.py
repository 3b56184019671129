"""GPU tests of the rectified-stereo post-processing chain (fsgm_stereo_sgm_pp_*, fsgm_stereo_disp_from_first_*,
fsgm_stereo_fb_check_*): every comparison is bit for bit against tests/stereo_pp_restatement.py -- same NaN positions, equal
values.  The inputs' non-vacuity is asserted in tests/test_stereo_pp_cpu.py; the shares are in its docstring."""
import ctypes as C
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, stereo_pp  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from tests import stereo_pp_restatement as P  # noqa: E402

pytestmark = pytest.mark.gpu
FSGM_ERR_INVALID = 1

# the row kernel's block is 256 threads: 255 / 256 / 257 are the widths around it, 513 and 1030 take several strides
WIDTHS = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1030]
HEIGHTS = [1, 2, 3, 5]
GEOMETRIES = list(itertools.product((0, -7, 40), (-1, +1)))
THRESHOLDS = (2.0, 0.0)
KINDS = ["random", "half", "constant", "two_plane", "nan_row", "all_nan"]
NAMES = ("disp_pp", "disp_checked", "disp", "minC", "disp2")


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype != np.float64:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    m = ~np.isnan(want)
    assert np.array_equal(got[m].view(np.uint64), want[m].view(np.uint64)), f"{what}: values differ"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stage_case(w, d_min, direction, what):
    """every form of the two stages on one map (or batch) against the restatement, frame by frame"""
    frames = w if w.ndim == 3 else w[None]
    D2want = np.stack([P.stereo_disp_from_first(f, d_min, direction) for f in frames]).reshape(w.shape)
    _same(fsgm_amd.stereo_disp_from_first(w, d_min, direction), D2want, f"{what}: second-view map")
    for thr in THRESHOLDS:
        want = np.stack([P.stereo_fb_check(f, d2, d_min, direction, thr) for f, d2 in zip(frames, D2want.reshape(frames.shape))]).reshape(w.shape)
        got, D2 = fsgm_amd.stereo_fb_check(w, None, d_min, direction, thr, return_second=True)      # the fused row kernel
        _same(got, want, f"{what} thr {thr}: fused check")
        _same(D2, D2want, f"{what} thr {thr}: fused second-view map")
        _same(fsgm_amd.stereo_fb_check(w, D2want, d_min, direction, thr), want, f"{what} thr {thr}: check against a given map")
    return D2want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_row_kernel_alone(gpu_lib, W, kind):
    for H in HEIGHTS:
        w = P.stage_maps(W, H)[kind]
        for d_min, direction in GEOMETRIES:
            _stage_case(w, d_min, direction, f"{kind} {W}x{H} d_min {d_min} direction {direction:+d}")


def test_row_kernel_at_the_widest_row(gpu_lib):
    W, H = 8192, 2
    w = P.stage_maps(W, H, dMax=200)["random"]
    _stage_case(w, -7, -1, "8192x2")
    assert stereo_pp.launch_lds(W) == 65536


@pytest.mark.parametrize("W,H", [(65, 3), (257, 2), (5, 1)])
def test_row_kernel_keeps_frames_apart(gpu_lib, W, H):
    n = 3
    w = np.stack([P.stage_maps(W, H, seed=11 + f)["random"] for f in range(n)])
    w[:-1, H - 1, :] = 23.0 + (np.arange(W) % 3)                 # the last row of frame f holds large values,
    w[1:, 0, :] = np.nan                                         # the first row of frame f + 1 nothing
    for d_min, direction in GEOMETRIES:
        D2 = _stage_case(w, d_min, direction, f"batch {W}x{H} d_min {d_min} direction {direction:+d}")
        assert (D2[1:, 0, :] == -1.0).all()


def test_stages_take_arbitrary_non_negative_doubles(gpu_lib):
    from fsgm_amd import synth
    W, H = 257, 5
    w = synth.uniform_f64(77, (H, W)) * 19.0 + 1.0 / 3.0         # no multiples of 1/256
    w[1, ::7] = np.nan
    w[2, 5], w[2, 6], w[3, 9], w[4, 0] = 1e18, np.inf, 5e-324, 0.0
    for d_min, direction in GEOMETRIES:
        _stage_case(w, d_min, direction, f"arbitrary doubles d_min {d_min} direction {direction:+d}")


def test_stages_report_a_negative_value(gpu_lib):
    w = P.stage_maps(65, 3)["random"]
    w[1, 7] = -0.25
    with pytest.raises(FsgmError) as e:
        fsgm_amd.stereo_disp_from_first(w)
    assert e.value.status == FSGM_ERR_INVALID
    out, status = torch_ops.stereo_fb_check(_t(w), return_status=True)
    assert out.is_cuda and int(status.item()) == FSGM_ERR_INVALID
    ok = np.nan_to_num(w, nan=1.0) >= 0
    out, second, status = torch_ops.stereo_fb_check(_t(np.where(ok, w, 0.0)), return_second=True, return_status=True)
    assert int(status.item()) == 0                               # the flag was cleared
    with pytest.raises(FsgmError):
        torch_ops.stereo_fb_check(_t(w), check=True)


def test_the_negative_flag_is_cleared_by_the_call_that_reports_it(gpu_lib):
    """D2=None (the row kernel raises the flag): FSGM_ERR_INVALID for one negative D1 value, and 0 from the very next call at the
    same shape on the same stream.  With D2 given no flag is read: 0 also for the negative value."""
    w = np.stack([P.stage_maps(9, 6, seed=31 + f)["constant"] for f in range(2)])
    bad = w.copy()
    bad[1, 2, 5] = -0.25
    status = [torch_ops.stereo_fb_check(_t(m), return_status=True)[-1] for m in (bad, w)]
    status.append(torch_ops.stereo_fb_check(_t(bad), _t(w), return_status=True)[-1])
    torch.cuda.synchronize()
    assert [int(s.item()) for s in status] == [FSGM_ERR_INVALID, 0, 0]


def test_stream_order_on_a_side_stream(gpu_lib):
    """inputs made by torch kernels on a side stream, the op, and torch ops on its outputs, with no synchronisation in between"""
    from fsgm_amd import synth
    W, H, D, n = 24, 16, 8, 2
    L, Rt = (np.stack(x) for x in zip(*[synth.image_pair(W, H, D, seed=51 + f) for f in range(n)]))
    want = fsgm_amd.stereo_sgm_pp(L, Rt, D)
    host = [torch.from_numpy(a).pin_memory() for a in (L, Rt)]
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        tL, tR = ((h.to("cuda:0", non_blocking=True).to(torch.int16) + 0).to(torch.uint8) for h in host)   # produced by kernels on s
        outs = torch_ops.stereo_sgm_pp(tL, tR, D)
        copies = [o.clone() for o in outs]
        tL.zero_()                                               # queued after the call: must not reach it
    s.synchronize()
    for g, w, name in zip(copies, want, NAMES):
        _same(g.cpu().numpy(), w, f"side stream {name}")


def test_torch_stage_equals_the_numpy_path(gpu_lib):
    w = np.stack([P.stage_maps(130, 5, seed=21 + f)["random"] for f in range(3)])
    tw = _t(w)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, D2 = torch_ops.stereo_fb_check(tw, None, -7, +1, 1.0, return_second=True)
        again = torch_ops.stereo_fb_check(tw, D2, -7, +1, 1.0)
    side.synchronize()
    assert got.is_cuda and D2.is_cuda and again.is_cuda
    want, D2want = fsgm_amd.stereo_fb_check(w, None, -7, +1, 1.0, return_second=True)
    _same(got.cpu().numpy(), want, "torch fused check")
    _same(D2.cpu().numpy(), D2want, "torch second-view map")
    _same(again.cpu().numpy(), want, "torch check against a given map")
    _same(torch_ops.stereo_fb_check(tw[1], None, -7, +1, 1.0).cpu().numpy(), want[1], "one frame")
    strided = torch.stack([D2, D2], dim=-1)[..., 0]               # D2 as a non-contiguous view: the op checks against a copy
    assert not strided.is_contiguous()
    _same(torch_ops.stereo_fb_check(tw, strided, -7, +1, 1.0).cpu().numpy(), want, "torch check against a non-contiguous map")


@pytest.mark.parametrize("call", P.CALLS, ids=P.call_id)
def test_whole_call(gpu_lib, call):
    key, n, paths, sub, ad, d_min, direction, fill, kw = call
    L, Rt, D, ref = P.call_reference(call)
    H, W = L.shape[-2:]
    args = dict(paths=paths, subpixel=sub, direction=direction, adaptive_p2=ad, d_min=d_min, in_fill=fill, **kw)
    # the host form, a batch or one frame
    host = fsgm_amd.stereo_sgm_pp(L if n > 1 else L[0], Rt if n > 1 else Rt[0], D, **args)
    assert [o.dtype for o in host] == [np.float64, np.float64, np.int32, np.uint32, np.float64]
    for k, name in enumerate(NAMES):
        got = host[k].reshape(n, H, W)
        for f in range(n):
            _same(got[f], ref[f][name], f"host {name} of frame {f}")
    if not fill:
        _same(host[0], host[1], "disp_pp without in-fill is disp_checked")
    # the matcher's raw outputs are stereo_sgm's own, before and after
    raw = fsgm_amd.stereo_sgm(L, Rt, D, paths=paths, subpixel=sub, direction=direction, adaptive_p2=ad, d_min=d_min)
    _same(host[2].reshape(n, H, W), raw[0], "disp vs stereo_sgm")
    _same(host[3].reshape(n, H, W), raw[1], "minC vs stereo_sgm")
    # the torch form on the current stream and on a side stream: outputs stay on the GPU
    tL, tR = _t(L), _t(Rt)
    outs = torch_ops.stereo_sgm_pp(tL, tR, D, return_status=True, **args)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        souts = torch_ops.stereo_sgm_pp(tL, tR, D, return_status=True, **args)
    side.synchronize()
    torch.cuda.current_stream().synchronize()
    assert int(outs[-1].item()) == 0 and int(souts[-1].item()) == 0
    for k, name in enumerate(NAMES):
        for o in (outs[k], souts[k]):
            assert o.is_cuda and tuple(o.shape) == (n, H, W)
            _same(o.cpu().numpy(), host[k].reshape(n, H, W), f"torch {name}")
    one = torch_ops.stereo_sgm_pp(tL[0], tR[0], D, check=True, **args)
    for k, name in enumerate(NAMES):
        assert one[k].is_cuda and tuple(one[k].shape) == (H, W)
        _same(one[k].cpu().numpy(), ref[0][name], f"torch {name}, one frame")
    # the device entry point with every optional output left out
    pp = stereo_pp.pp_params(gpu_lib, fill, kw)
    prm = fsgm_amd.epi._stereo_params(paths, sub, direction, 0, 0)
    opt = fsgm_amd._lib.options(ad)
    only = torch.full((n, H, W), 7.0, dtype=torch.float64, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    torch.cuda.synchronize()
    st = gpu_lib.fsgm_stereo_sgm_pp_device(n, p(tL), p(tR), W, H, D, 6, 64, C.byref(prm), C.byref(opt), d_min, C.byref(pp), p(only), None,
                                           None, None, None, None, None)
    assert st == 0, gpu_lib.fsgm_last_error()
    torch.cuda.synchronize()
    _same(only.cpu().numpy(), host[0].reshape(n, H, W), "device form, disp_pp alone")


def test_device_form_refuses_host_memory_and_fb_check(gpu_lib):
    call = P.CALLS[0]
    L, Rt, D, _ = P.call_reference(call)
    H, W = L.shape[-2:]
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm_pp(torch.from_numpy(L[0]), _t(Rt[0]), D)
    dL, dR = _t(L), _t(Rt)
    out = torch.full((1, H, W), 7.0, dtype=torch.float64, device="cuda:0")
    pinned = torch.from_numpy(L).pin_memory()
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    st = gpu_lib.fsgm_stereo_sgm_pp_device(1, p(pinned), p(dR), W, H, D, 6, 64, None, None, 0, None, p(out), None, None, None, None, None, None)
    assert st == FSGM_ERR_INVALID
    prm = gpu_lib.fsgm_stereo_params_default()
    prm.fb_check = 1
    st = gpu_lib.fsgm_stereo_sgm_pp_device(1, p(dL), p(dR), W, H, D, 6, 64, C.byref(prm), None, 0, None, p(out), None, None, None, None, None, None)
    assert st == FSGM_ERR_INVALID and b"fb_check" in gpu_lib.fsgm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
