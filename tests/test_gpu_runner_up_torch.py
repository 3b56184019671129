"""GPU tests of fsgm::stereo_sgm_ru / torch_ops.stereo_sgm(runner_up=True) and fsgm::uniqueness_filter against the numpy forms,
and of the device-pointer contract of fsgm_stereo_sgm_device_ru and fsgm_uniqueness_filter_device: the caller's stream, tensors read
where they lie at any byte address, foreign memory refused before anything is queued, a captured stream refused."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from tests import runner_up_restatement as RU  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4


def _t(a, dev="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.cpu().numpy()


def _odd(a):
    """the array as a slice of a uint8 tensor that starts at an odd byte address"""
    buf = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda:0")
    buf[1:] = _t(a).reshape(-1)
    t = buf[1:].view(a.shape)
    assert t.data_ptr() % 2 == 1
    return t


@pytest.mark.parametrize("fb,d_min,D", [(0, -3, 64), (1, None, 48), (1, 5, 20)])
def test_torch_stereo_runner_up_equals_the_numpy_path(gpu_lib, fb, d_min, D):
    W, H, n = 61, 17, 3
    pairs = [synth.image_pair(W, H, D, seed=60 + f) for f in range(n)]
    L, Rt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = fsgm_amd.stereo_sgm(L, Rt, D, paths=8, fb_check=fb, d_min=d_min, runner_up=True)
    plain = fsgm_amd.stereo_sgm(L, Rt, D, paths=8, fb_check=fb, d_min=d_min)
    tL, tR = _odd(L), _odd(Rt)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # a non-default stream
        outs = torch_ops.stereo_sgm(tL, tR, D, paths=8, fb_check=fb, d_min=d_min, runner_up=True, return_status=True)
    side.synchronize()
    assert int(outs[-1].item()) == 0 and len(outs) == len(want) + 1 == len(plain) + 2
    for k, w in enumerate(want):
        assert outs[k].is_cuda and outs[k].shape == (n, H, W) and _n(outs[k]).dtype == w.dtype
        np.testing.assert_array_equal(_n(outs[k]), w, err_msg=f"output {k}: torch vs host entry point")
    for k, w in enumerate(plain):
        np.testing.assert_array_equal(_n(outs[k]), w, err_msg=f"output {k}: with and without runner_up")
    one = torch_ops.stereo_sgm(tL[1], tR[1], D, paths=8, fb_check=fb, d_min=d_min, runner_up=True, check=True)
    for k, w in enumerate(want):
        assert one[k].shape == (H, W)
        np.testing.assert_array_equal(_n(one[k]), w[1], err_msg=f"output {k}: one frame")


@pytest.mark.parametrize("ratio", [0, 15, 100])
def test_torch_uniqueness_filter(gpu_lib, ratio):
    rng = np.random.default_rng(3 + ratio)
    shape = (2, 19, 37)
    m = rng.uniform(0, 64, shape)
    m[rng.random(shape) < 0.2] = np.nan
    minC = rng.integers(1, 2041, shape).astype(np.uint32)
    minC2 = (minC + rng.integers(0, 400, shape)).astype(np.uint32)
    minC2[rng.random(shape) < 0.1] = RU.NO_RUNNER_UP
    big = rng.random(shape) < 0.2
    minC2[big] = 2 ** 32 // 100 + 7
    minC[big] = 2 ** 32 // 100 - 3
    want = RU.uniqueness_filter(m, minC, minC2, ratio)
    tm, tc, tc2 = _t(m), _t(minC), _t(minC2)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = torch_ops.uniqueness_filter(tm, tc, tc2, ratio)
    side.synchronize()
    assert got.is_cuda and got.dtype == torch.float64 and got.data_ptr() != tm.data_ptr()
    assert np.array_equal(_n(got), want, equal_nan=True) and np.array_equal(_n(tm), m, equal_nan=True)
    assert np.array_equal(_n(torch_ops.uniqueness_filter(tm[1], tc[1], tc2[1], ratio)), want[1], equal_nan=True)
    # a strided view goes in as a contiguous copy
    wide = torch.zeros((2, 19, 40), dtype=torch.float64, device="cuda:0")
    wide[..., :37] = tm
    assert np.array_equal(_n(torch_ops.uniqueness_filter(wide[..., :37], tc, tc2, ratio)), want, equal_nan=True)
    # in place at the entry point, on the current stream
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    status = torch.full((), 7, dtype=torch.int32, device="cuda:0")
    inplace = tm.clone()
    st = gpu_lib.fsgm_uniqueness_filter_device(2, p(inplace), p(tc), p(tc2), 37, 19, ratio, p(inplace), 0,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream), p(status))
    torch.cuda.synchronize()
    assert st == 0 and int(status.item()) == 0 and np.array_equal(_n(inplace), want, equal_nan=True)


def test_foreign_memory_is_refused_before_anything_is_queued(gpu_lib):
    W, H, D = 24, 9, 16
    I1, I2 = synth.image_pair(W, H, D)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(torch.from_numpy(I1), _t(I2), D, runner_up=True)
    dI1, dI2 = _t(I1), _t(I2)
    full = lambda dev="cuda:0": torch.full((H, W), 7, dtype=torch.int32, device=dev)   # noqa: E731
    disp, minC, minC2 = full(), full(), full()
    pinned = torch.full((H, W), 7, dtype=torch.int32).pin_memory()
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    call = lambda m2: gpu_lib.fsgm_stereo_sgm_device_ru(1, p(dI1), p(dI2), W, H, D, 6, 64, None, None, 3, p(disp), p(minC), m2, None, None,   # noqa: E731
                                                         None, None)
    assert call(p(pinned)) == INVALID and b"minC2" in gpu_lib.fsgm_last_error()
    assert call(None) == INVALID and b"minC2" in gpu_lib.fsgm_last_error()
    assert call(C.c_void_p(minC2.data_ptr() + 2)) == INVALID and b"minC2" in gpu_lib.fsgm_last_error()      # misaligned
    if torch.cuda.device_count() > 1:
        other = full("cuda:1")
        assert call(p(other)) == INVALID and b"minC2" in gpu_lib.fsgm_last_error()
    m = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
    st = gpu_lib.fsgm_uniqueness_filter_device(1, p(m), p(minC), p(pinned), W, H, 15, p(m), 0, None, None)
    assert st == INVALID and b"minC2" in gpu_lib.fsgm_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (disp, minC, minC2)) and bool((pinned == 7).all())
    assert call(p(minC2)) == 0                                    # the same call with its own memory runs
    torch.cuda.synchronize()
    assert not bool((minC2 == 7).all())


def test_graph_capture_is_refused(gpu_lib):
    W, H, D = 32, 24, 16
    L, R = (_t(a) for a in synth.image_pair(W, H, D, seed=32))
    disp, minC, minC2 = torch_ops.stereo_sgm(L, R, D, runner_up=True, check=True)
    m = torch.ones((H, W), dtype=torch.float64, device="cuda:0")
    torch_ops.uniqueness_filter(m, minC, minC2, 15)
    torch.cuda.synchronize()
    for work in (lambda: torch_ops.stereo_sgm(L, R, D, runner_up=True), lambda: torch_ops.uniqueness_filter(m, minC, minC2, 15)):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(FsgmError) as ei:
            with torch.cuda.graph(g):
                work()
        assert ei.value.status == UNSUPPORTED and "captured" in str(ei.value)
