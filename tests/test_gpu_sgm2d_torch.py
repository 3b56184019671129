"""GPU tests of fsgm::sgm2d / torch_ops.sgm2d and of fsgm_sgm2d_device's contract: the tensor read where it lies in each layout,
at any byte address, ordered on the caller's stream, refused while that stream is captured, the saturation word in the status."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, synth, sgm2d_batch, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd.sgm2d import _bind, params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
LAYOUTS = ("hwd", "dhw", "dhw_yx")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(W, H, rX, rY, n, seed, cmax=24, larger=True):
    """(volumes (n, H, W, D) in reference order, hints (n, 2, mvH, mvW), guide (n, H, W))"""
    D = (2 * rX + 1) * (2 * rY + 1)
    vols = np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])
    mvW, mvH = (W + 2, H + 1) if larger else (W, H)
    hints = np.stack([synth.hint_map(mvW, mvH, "general", seed=seed + 5 * f, amp=3.0) for f in range(n)])
    guide = np.stack([synth.image_pair(W, H, 16, seed=seed + f)[0] // 2 for f in range(n)])
    guide[:, :, W // 2:] += 120
    return vols, hints, guide


def _as(layout, vols, Sx, Sy):
    n, H, W, D = vols.shape
    if layout == "hwd":
        return vols
    if layout == "dhw":
        return np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(vols.reshape(n, H, W, Sx, Sy).transpose(0, 4, 3, 1, 2).reshape(n, D, H, W))


def _equal(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("bestD", "minC", "mvSub", "flow", "S")):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rX,rY,bound,adaptive", [(4, 4, 24, 0), (1, 2, 24, 1), (6, 4, 255, 0), (6, 4, 24, 1)])
def test_the_op_equals_the_host_form_on_the_same_bytes(gpu_lib, layout, rX, rY, bound, adaptive):
    W, H, n = 40, 12, 3
    vols, hints, guide = _case(W, H, rX, rY, n, seed=3, cmax=bound)
    src = _as(layout, vols, 2 * rX + 1, 2 * rY + 1)
    kw = dict(layout=layout, cost_bound=bound, adaptive_p2=adaptive, return_flow=True, return_sum=True)
    want = sgm2d_batch(src, rX, rY, 6, 32, hints=hints, guide=guide if adaptive else None, **kw)
    got = torch_ops.sgm2d(_t(src), rX, rY, 6, 32, hints=_t(hints), guide=_t(guide) if adaptive else None, check=True, **kw)
    assert [g.dtype for g in got] == [torch.uint32, torch.uint32, torch.float64, torch.float64, torch.uint32]
    assert all(g.device.type == "cuda" for g in got)
    _equal(got, want, layout)
    # one volume without the batch axis, no hints
    want = sgm2d_batch(src[0], rX, rY, 6, 32, layout=layout, cost_bound=bound)
    _equal(torch_ops.sgm2d(_t(src[0]), rX, rY, 6, 32, layout=layout, cost_bound=bound), want, f"{layout} single")


def test_a_tensor_that_is_not_contiguous_uint8_raises(gpu_lib):
    vols, hints, _ = _case(40, 12, 1, 2, 2, seed=5)
    Ct = _t(vols)                                               # (n, H, W, D)
    with pytest.raises(TypeError, match="contiguous"):
        torch_ops.sgm2d(Ct.permute(0, 3, 1, 2), 1, 2, layout="dhw")
    with pytest.raises(TypeError, match="contiguous"):
        torch.ops.fsgm.sgm2d(Ct.permute(0, 3, 1, 2), torch.empty(0, dtype=torch.float64, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV),
                             1, 2, 6, 32, 1, 255, 1, 2, 0, 1, 0, 0)
    with pytest.raises(TypeError, match="uint8"):
        torch_ops.sgm2d(Ct.to(torch.int16), 1, 2, layout="hwd")
    with pytest.raises(TypeError, match="uint8"):
        torch_ops.sgm2d(Ct.float(), 1, 2, layout="hwd")
    with pytest.raises(TypeError, match="float64"):
        torch_ops.sgm2d(Ct, 1, 2, layout="hwd", hints=_t(hints).float())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stream_order_on_a_side_stream(gpu_lib, layout):
    """the costs filled by torch kernels on a side stream just before the call on that stream, the outputs consumed on it, no
    device synchronisation in between"""
    W, H, n, rX, rY = 160, 96, 2, 4, 4
    vols, hints, _ = _case(W, H, rX, rY, n, seed=11)
    src = _as(layout, vols, 9, 9)
    ref = torch_ops.sgm2d(_t(src), rX, rY, hints=_t(hints), layout=layout, cost_bound=24, return_flow=True, check=True)
    torch.cuda.synchronize()
    host, hhost = torch.from_numpy(src).pin_memory(), torch.from_numpy(hints).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Ct = torch.zeros(src.shape, dtype=torch.uint8, device=DEV)
        up = host.to(DEV, non_blocking=True)
        Ct.copy_((up.to(torch.int16) + 0).to(torch.uint8))          # filled by kernels on s
        Ht = hhost.to(DEV, non_blocking=True) * 1.0
        bd, mc, ms, fl = torch_ops.sgm2d(Ct, rX, rY, hints=Ht, layout=layout, cost_bound=24, return_flow=True)
        kept = [t.clone() for t in (bd, mc, ms, fl)]                # consumed on s
        Ct.zero_()                                                  # queued after the call: must not reach it
        Ht.zero_()
    s.synchronize()
    for k, r in zip(kept, ref):
        assert torch.equal(k, r)


def test_a_capturing_stream_is_refused_and_nothing_is_allocated(gpu_lib):
    """through the C entry, with hipStreamBeginCapture in relaxed mode, on a shape no plan exists for"""
    lib = _bind(_lib.load())
    hip = C.CDLL(torch_ops.hip_runtimes()[0])
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    W, H, n, rX, rY = 161, 97, 2, 2, 1                              # (a shape of this test's own: its plan would take 6 MB)
    NP, D = W * H, 15
    Ct = torch.zeros(n * NP * D, dtype=torch.uint8, device=DEV)
    out = torch.full((2 * n * NP,), 0xABCD, dtype=torch.int32, device=DEV)
    sub = torch.full((2 * n * NP,), -7.0, dtype=torch.float64, device=DEV)
    prm = params(lib, layout="dhw")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def free():
        a, b = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value

    def call():
        return lib.fsgm_sgm2d_device(n, C.c_void_p(Ct.data_ptr()), W, H, rX, rY, 6, 32, C.byref(prm), None, 0, 0, None,
                                     C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 4 * n * NP), C.c_void_p(sub.data_ptr()), None, None,
                                     C.c_void_p(s.cuda_stream), None)
    def captured(work):
        """work() between begin and end of a relaxed capture of s; the device memory the whole cycle took"""
        before = free()
        assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0      # hipStreamCaptureModeRelaxed
        try:
            res = work()
        finally:
            graph = C.c_void_p()
            assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph)) == 0
            if graph:
                hip.hipGraphDestroy(graph)
        return res, before - free()

    # (the runtime takes memory of its own for a stream's first capture: the yardstick is an empty capture behind a first one)
    captured(lambda: None)
    _, empty = captured(lambda: None)
    (st, err), taken = captured(lambda: (call(), lib.fsgm_last_error().decode()))
    assert st == FSGM_ERR_UNSUPPORTED and "captured" in err
    assert taken == empty, "a refused call allocated device memory"
    torch.cuda.synchronize()
    assert bool((out == 0xABCD).all()) and bool((sub == -7.0).all()), "a refused call queued something"
    assert call() == 0                                              # the same call outside the capture runs
    s.synchronize()
    assert not bool((out == 0xABCD).all())


def test_return_status_carries_the_saturation_word(gpu_lib):
    vols, _, _ = _case(40, 12, 4, 4, 2, seed=12)
    over = vols.copy()
    over[1, 3, 4, 9] = 200
    status = [torch_ops.sgm2d(_t(_as("dhw_yx", v, 9, 9)), 4, 4, layout="dhw_yx", cost_bound=24, return_status=True)[-1] for v in (over, vols)]
    torch.cuda.synchronize()
    assert [int(s.item()) for s in status] == [FSGM_ERR_INVALID, 0]      # raised, and cleared by the call that reported it
    assert status[0].dtype == torch.int32 and status[0].dim() == 0
    with pytest.raises(_lib.FsgmError) as e:
        torch_ops.sgm2d(_t(_as("dhw_yx", over, 9, 9)), 4, 4, layout="dhw_yx", cost_bound=24, check=True)
    assert e.value.status == FSGM_ERR_INVALID


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H,rX,rY,n", [(67, 5, 4, 4, 3), (33, 5, 1, 2, 1), (64, 1, 6, 4, 1), (131, 5, 2, 1, 2), (9, 7, 15, 16, 1)])
def test_an_unaligned_source_equals_the_aligned_run(gpu_lib, layout, W, H, rX, rY, n):
    """u8 has no alignment rule: a view starting one byte into a larger allocation, which the pointer check must accept"""
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    vols, hints, _ = _case(W, H, rX, rY, n, seed=5, cmax=255, larger=False)
    src = _as(layout, vols, Sx, Sy)
    big = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    big[1:] = _t(src).reshape(-1)
    view = big[1:].view(src.shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    kw = dict(layout=layout, hints=_t(hints), cost_bound=100, return_flow=True, return_sum=True, return_status=True)
    aligned = torch_ops.sgm2d(_t(src), rX, rY, 6, 32, **kw)
    odd = torch_ops.sgm2d(view, rX, rY, 6, 32, **kw)
    torch.cuda.synchronize()
    for a, b in zip(aligned, odd):
        assert torch.equal(a, b)
    assert int(odd[-1].item()) == FSGM_ERR_INVALID                     # costs up to 255 under a bound of 100: saturated alike
