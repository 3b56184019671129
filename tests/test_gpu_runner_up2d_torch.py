"""GPU tests of fsgm::sgm2d_ru, fsgm::sgm_ru and fsgm::uniqueness_filter_planes: CUDA tensors against the numpy forms (themselves
held to the oracle by tests/test_gpu_runner_up2d.py), a non-default stream, the status word, and the refusal of a stream under
capture -- asserted alone: no graph is ever replayed."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, synth, sgm2d_batch, sgm_batch  # noqa: E402  (torch first, then the library)
import fsgm_amd  # noqa: E402
from fsgm_amd._lib import FsgmError  # noqa: E402
from tests import runner_up_restatement as RU  # noqa: E402
from tests import runner_up2d_restatement as RU2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID, UNSUPPORTED = 1, 4
W, H = 21, 10


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _as(layout, vols):
    n = vols.shape[0]
    if layout == "dhw":
        return np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(vols.reshape(n, H, W, 9, 9).transpose(0, 4, 3, 1, 2).reshape(n, 81, H, W))


def _volumes(n, D, seed, cmax=24):
    return np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])


@pytest.mark.parametrize("layout", ["dhw", "dhw_yx"])
@pytest.mark.parametrize("n", [1, 3])
def test_sgm2d_ru(gpu_lib, n, layout):
    vols = _volumes(n, 81, seed=n)
    hints = np.stack([synth.hint_map(W, H, "general", seed=40 + f, amp=3.0) for f in range(n)])
    kw = dict(layout=layout, hints=hints, cost_bound=24, return_flow=True, return_sum=True)
    want = sgm2d_batch(_as(layout, vols), 4, 4, runner_up=True, **kw)
    np.testing.assert_array_equal(want[2], RU2.runner_up2d(want[5], 9, 9)[2])
    kw["hints"] = _t(hints)
    got = torch_ops.sgm2d(_t(_as(layout, vols)), 4, 4, runner_up=True, check=True, **kw)
    plain = torch_ops.sgm2d(_t(_as(layout, vols)), 4, 4, check=True, **kw)
    assert len(got) == 6 and len(plain) == 5
    for g, w in zip(got, want):
        assert g.device == torch.device(DEV)
        np.testing.assert_array_equal(_n(g), w)
    for g, p in zip(got[:2] + got[3:], plain):
        assert torch.equal(g, p)
    assert got[2].dtype == torch.uint32
    one = torch_ops.sgm2d(_t(_as(layout, vols))[0], 4, 4, runner_up=True, layout=layout, hints=kw["hints"][0], cost_bound=24)
    assert len(one) == 4 and tuple(one[2].shape) == (H, W)
    np.testing.assert_array_equal(_n(one[2]), want[2][0])


@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("n", [1, 3])
def test_sgm_ru(gpu_lib, n, layout):
    vols = _volumes(n, 48, seed=7 + n)
    src = vols if layout == "hwd" else np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    want = sgm_batch(src, 7, 100, layout=layout, cost_bound=24, runner_up=True, return_sum=True)
    np.testing.assert_array_equal(want[2], RU.runner_up(want[3])[2])
    got = torch_ops.sgm(_t(src), 7, 100, layout=layout, cost_bound=24, runner_up=True, return_sum=True, check=True)
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.device == torch.device(DEV)
        np.testing.assert_array_equal(_n(g), w)
    plain = torch_ops.sgm(_t(src), 7, 100, layout=layout, cost_bound=24, check=True)
    assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    with pytest.raises(FsgmError) as e:
        torch_ops.sgm(_t(src), 7, 100, layout=layout, cost_bound=24, runner_up=True, agg_mode=4)
    assert e.value.status == UNSUPPORTED


def _filter_inputs(n):
    rng = np.random.default_rng(n)
    minC = rng.integers(0, 2041, (n, H, W)).astype(np.uint32)
    minC2 = np.maximum(minC, rng.integers(0, 2300, (n, H, W))).astype(np.uint32)
    minC2.flat[::7] = RU.NO_RUNNER_UP
    minC2.flat[3::13] = 0xFFFFFFFE
    flow = rng.normal(0, 3, (n, 2, H, W))
    flow[:, 1].flat[::9] = np.nan
    return flow, minC, minC2


@pytest.mark.parametrize("ratio", [0, 15, 100])
@pytest.mark.parametrize("n", [1, 3])
def test_uniqueness_filter_planes(gpu_lib, n, ratio):
    flow, minC, minC2 = _filter_inputs(n)
    want = fsgm_amd.uniqueness_filter(flow, minC, minC2, ratio, planes=2)
    np.testing.assert_array_equal(want, RU2.uniqueness_filter_flow(flow, minC, minC2, ratio))
    f, c, c2 = _t(flow), _t(minC), _t(minC2)
    out = torch_ops.uniqueness_filter(f, c, c2, ratio, planes=2)
    assert out.device == f.device and out.data_ptr() != f.data_ptr()
    np.testing.assert_array_equal(_n(out), want)
    np.testing.assert_array_equal(_n(f), flow)                   # the input is left alone
    np.testing.assert_array_equal(_n(torch_ops.uniqueness_filter(f[0], c[0], c2[0], ratio, planes=2)), want[0])
    raw, status = torch.ops.fsgm.uniqueness_filter_planes(f, c, c2, ratio, 2)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    np.testing.assert_array_equal(_n(raw), want)
    for bad_map, planes in ((f[:, 0].contiguous(), 2), (f, 1), (f[:, :, :-1].contiguous(), 2)):      # the raw op checks its shapes
        with pytest.raises(TypeError, match="map_ must be"):
            torch.ops.fsgm.uniqueness_filter_planes(bad_map, c, c2, ratio, planes)
    with pytest.raises(ValueError, match="planes"):
        torch.ops.fsgm.uniqueness_filter_planes(f, c, c2, ratio, 3)
    one, _ = torch.ops.fsgm.uniqueness_filter_planes(f[:, 0].contiguous(), c, c2, ratio, 1)
    old, _ = torch.ops.fsgm.uniqueness_filter(f[:, 0].contiguous(), c, c2, ratio)
    assert _n(one).tobytes() == _n(old).tobytes()


def test_non_default_stream(gpu_lib):
    vols = _volumes(3, 81, seed=5)
    want = sgm2d_batch(_as("dhw", vols), 4, 4, layout="dhw", cost_bound=24, runner_up=True, return_flow=True)
    s = torch.cuda.Stream(device=DEV)
    src = _t(_as("dhw", vols))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        bd, mc, m2, ms, flow = torch_ops.sgm2d(src, 4, 4, layout="dhw", cost_bound=24, runner_up=True, return_flow=True)
        kept = torch_ops.uniqueness_filter(flow, mc, m2, 15, planes=2)
    s.synchronize()
    for g, w in zip((bd, mc, m2, ms, flow), want):
        np.testing.assert_array_equal(_n(g), w)
    np.testing.assert_array_equal(_n(kept), RU2.uniqueness_filter_flow(want[4], want[1], want[2], 15))


def test_status_and_check(gpu_lib):
    """as fsgm::sgm2d: a cost above the declared bound is saturated on the way in and reported in the status word"""
    vols = _volumes(1, 81, seed=3)
    vols[0, 4, 5, 6] = 200
    src = _t(_as("dhw", vols))
    *got, st = torch_ops.sgm2d(src, 4, 4, layout="dhw", cost_bound=24, runner_up=True, return_status=True)
    torch.cuda.synchronize()
    assert int(st.item()) == INVALID and len(got) == 4
    want = sgm2d_batch(np.minimum(_as("dhw", vols), 24), 4, 4, layout="dhw", cost_bound=24, runner_up=True)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_n(g), w)
    with pytest.raises(FsgmError) as e:
        torch_ops.sgm2d(src, 4, 4, layout="dhw", cost_bound=24, runner_up=True, check=True)
    assert e.value.status == INVALID
    *_, st = torch_ops.sgm2d(src, 4, 4, layout="dhw", cost_bound=255, runner_up=True, return_status=True)
    torch.cuda.synchronize()
    assert int(st.item()) == 0


def test_captured_stream_is_refused(gpu_lib):
    """UNSUPPORTED before anything is queued, through the C entries with hipStreamBeginCapture in relaxed mode, as
    tests/test_gpu_sgm2d_torch.py does it; the capture is ended and its graph destroyed, never instantiated or replayed"""
    import ctypes as C
    import importlib
    from fsgm_amd import _lib
    from fsgm_amd.sgm2d import _bind as bind2d, params as params2d
    sgm1d = importlib.import_module("fsgm_amd.sgm")
    lib = sgm1d._bind(bind2d(_lib.load()))
    hip = C.CDLL(torch_ops.hip_runtimes()[0])
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    NP = W * H
    vols2d, vols1d = _t(_as("dhw", _volumes(1, 81, seed=9))), _t(_volumes(1, 16, seed=9))
    flow, minC, minC2 = (_t(a) for a in _filter_inputs(1))
    u32 = torch.full((3 * NP,), 0xABCD, dtype=torch.int32, device=DEV)
    f64 = torch.full((4 * NP,), -7.0, dtype=torch.float64, device=DEV)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)          # noqa: E731
    prm2d, prm1d = params2d(lib, layout="dhw", cost_bound=24), sgm1d.params(lib, layout="hwd", cost_bound=24)
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    calls = [lambda: lib.fsgm_sgm2d_device_ru(1, p(vols2d), W, H, 4, 4, 6, 32, C.byref(prm2d), None, 0, 0, None, p(u32), p(u32, 4 * NP),
                                              p(u32, 8 * NP), p(f64), None, None, st, None),
             lambda: lib.fsgm_sgm_device_ru(1, p(vols1d), W, H, 16, 7, 100, C.byref(prm1d), None, p(u32), p(u32, 4 * NP), p(u32, 8 * NP),
                                            None, st, None),
             lambda: lib.fsgm_uniqueness_filter_planes_device(1, p(flow), p(minC), p(minC2), W, H, 2, 15, p(f64), 0, st, None)]
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(st, 2) == 0                 # hipStreamCaptureModeRelaxed
    try:
        res = [(call(), lib.fsgm_last_error().decode()) for call in calls]
    finally:
        graph = C.c_void_p()
        assert hip.hipStreamEndCapture(st, C.byref(graph)) == 0
        if graph:
            hip.hipGraphDestroy(graph)
    torch.cuda.synchronize()
    for status, err in res:
        assert status == UNSUPPORTED and "captured" in err
    assert bool((u32 == 0xABCD).all()) and bool((f64 == -7.0).all()), "a refused call queued something"
    assert [call() for call in calls] == [0, 0, 0]               # the same calls outside the capture run
    s.synchronize()
    assert not bool((u32 == 0xABCD).all()) and not bool((f64 == -7.0).all())
