"""GPU tests of fsgm::sgm2d_exact (torch_ops.sgm2d(arith="exact"), fsgm_sgm2d_device_exact): tensors in HBM in and out on the
caller's stream against the restatement of tests/sgm2d_exact_restatement.py, with and without the runner-up cost; a side stream, a
tensor that is not contiguous, an odd base address, the op's schema and fake, and the refusal of a stream under capture --
asserted alone: no graph is ever instantiated or replayed."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd.sgm2d import _bind, last_kernel, params  # noqa: E402
from tests import sgm2d_exact_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_UNSUPPORTED = 4
NAMES = ("bestD", "minC", "mvSub", "flow", "S", "minC2")
# a rows-layout window with adaptive P2 and hints beyond the window, and a compact one
CASES = [K.Case(21, 13, 4, 4, 3, 7, 100, "dhw_yx", "beyond", 1, 1, 2, 1, "random"),
         K.Case(21, 13, 6, 6, 2, 20, 200, "dhw", "general", 0, 1, 2, 1, "random")]


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are read-only)


def _call(c, Ct, hints, guides, runner_up, **kw):
    """(bestD, minC, mvSub, flow, S[, minC2]) of torch_ops.sgm2d(arith="exact") on the case's switches; tensors"""
    out = torch_ops.sgm2d(Ct, c.rX, c.rY, c.P1, c.P2, layout=c.layout, hints=hints, guide=guides, diagonal=c.diagonal, total_pass=c.passes,
                          adaptive_p2=c.adaptive, subpixel=c.subpixel, return_flow=True, return_sum=True, arith="exact", runner_up=runner_up,
                          **kw)
    return (out[0], out[1]) + tuple(out[3:]) + (out[2],) if runner_up else out


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, NAMES):
        assert g.is_cuda
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}"
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _src(c):
    vols, hints, guides = K.inputs(c)
    return K.as_layout(c.layout, vols, 2 * c.rX + 1, 2 * c.rY + 1), hints, guides


@pytest.mark.parametrize("runner_up", [False, True], ids=["plain", "minC2"])
@pytest.mark.parametrize("c", CASES, ids=K.case_id)
def test_the_op_against_the_restatement(gpu_lib, c, runner_up):
    src, hints, guides = _src(c)
    want = K.want(c)[:6 if runner_up else 5]
    _same(_call(c, _t(src), _t(hints), _t(guides), runner_up, check=True), want, "batch")
    assert last_kernel() == "generic/exact"
    # one volume without the batch axis
    one = _call(c, _t(src[0]), _t(hints[0]), None if guides is None else _t(guides[0]), runner_up, check=True)
    _same(one, tuple(w[0] for w in want), "single")


@pytest.mark.parametrize("runner_up", [False, True], ids=["plain", "minC2"])
@pytest.mark.parametrize("c", CASES, ids=K.case_id)
def test_on_a_side_stream(gpu_lib, c, runner_up):
    """the costs and hints filled by torch kernels on a side stream just before the call on that stream, the outputs consumed on
    it, the inputs cleared right behind the call: no device synchronisation in between"""
    src, hints, guides = _src(c)
    want = K.want(c)[:6 if runner_up else 5]
    _call(c, _t(src), _t(hints), _t(guides), runner_up, check=True)                    # the shape is warm
    torch.cuda.synchronize()
    host, hhost = torch.from_numpy(np.array(src)).pin_memory(), torch.from_numpy(np.array(hints)).pin_memory()
    Gt = _t(guides)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Ct = torch.zeros(src.shape, dtype=torch.uint8, device=DEV)
        Ct.copy_((host.to(DEV, non_blocking=True).to(torch.int16) + 0).to(torch.uint8))       # filled by kernels on s
        Ht = hhost.to(DEV, non_blocking=True) * 1.0
        kept = [t.clone() for t in _call(c, Ct, Ht, Gt, runner_up)]                    # consumed on s
        Ct.zero_()                                                                     # queued after the call: must not reach it
        Ht.zero_()
    s.synchronize()
    _same(kept, want, "side stream")


@pytest.mark.parametrize("runner_up", [False, True], ids=["plain", "minC2"])
def test_a_tensor_that_is_not_contiguous_raises(gpu_lib, runner_up):
    c = CASES[1]
    vols, _, _ = K.inputs(c)
    Ct = _t(vols)                                                # (n, H, W, D): its permutation has the "dhw" shape and no copy
    with pytest.raises(TypeError, match="contiguous"):
        torch_ops.sgm2d(Ct.permute(0, 3, 1, 2), c.rX, c.rY, layout="dhw", arith="exact", runner_up=runner_up)
    with pytest.raises(TypeError, match="contiguous"):
        torch.ops.fsgm.sgm2d_exact(Ct.permute(0, 3, 1, 2), torch.empty(0, dtype=torch.float64, device=DEV),
                                   torch.empty(0, dtype=torch.uint8, device=DEV), c.rX, c.rY, 7, 100, 1, 255, 1, 2, 0, 1, 0, 0, runner_up)
    with pytest.raises(TypeError, match="uint8"):
        torch_ops.sgm2d(Ct.to(torch.int16), c.rX, c.rY, layout="hwd", arith="exact", runner_up=runner_up)


@pytest.mark.parametrize("runner_up", [False, True], ids=["plain", "minC2"])
@pytest.mark.parametrize("c", CASES, ids=K.case_id)
def test_an_unaligned_base_address(gpu_lib, c, runner_up):
    """u8 has no alignment rule: a view starting one byte into a larger allocation, which the pointer check must accept"""
    src, hints, guides = _src(c)
    big = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    big[1:] = _t(src).reshape(-1)
    view = big[1:].view(src.shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    _same(_call(c, view, _t(hints), _t(guides), runner_up, check=True), K.want(c)[:6 if runner_up else 5], "unaligned")


def test_schema_and_fake(gpu_lib):
    c = CASES[0]
    src, hints, guides = _src(c)
    code = {"hwd": 0, "dhw": 1, "dhw_yx": 2}[c.layout]
    checks = ("test_schema", "test_faketensor")
    for runner_up in (False, True):
        args = (_t(src), _t(hints), _t(guides), c.rX, c.rY, c.P1, c.P2, code, 255, 1, 2, 1, 1, 1, 1, runner_up)
        torch.library.opcheck(torch.ops.fsgm.sgm2d_exact.default, args, test_utils=checks)
        out = torch.ops.fsgm.sgm2d_exact(*args)
        assert tuple(out[2].shape) == ((c.n, c.H, c.W) if runner_up else (0,)) and out[2].dtype == torch.uint32
    # neither flow nor S nor hints: empty tensors out, as fsgm::sgm2d_ru returns them
    out = torch.ops.fsgm.sgm2d_exact(_t(src), torch.empty(0, dtype=torch.float64, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV),
                                     c.rX, c.rY, c.P1, c.P2, code, 255, 1, 2, 0, 1, 0, 0, False)
    assert [o.numel() for o in out[2:6]] == [0, 2 * c.n * c.H * c.W, 0, 0]


def test_a_capturing_stream_is_refused_not_queued(gpu_lib):
    """FSGM_ERR_UNSUPPORTED before anything is queued, through the C entry with hipStreamBeginCapture in relaxed mode, as
    tests/test_gpu_sgm2d_torch.py does it; the capture is ended and its graph destroyed, never instantiated or replayed"""
    lib = _bind(_lib.load())
    hip = C.CDLL(torch_ops.hip_runtimes()[0])
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    W, H, rX, rY, n = 19, 11, 3, 3, 1                            # a shape no other test uses: no plan exists for it
    NP = W * H
    Ct = _t(K.volumes(W, H, 49, n, 77).transpose(0, 3, 1, 2))
    u32 = torch.full((3 * NP,), 0xABCD, dtype=torch.int32, device=DEV)
    f64 = torch.full((2 * NP,), -7.0, dtype=torch.float64, device=DEV)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)          # noqa: E731
    prm = params(lib, layout="dhw")
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    calls = [lambda: lib.fsgm_sgm2d_device_exact(n, p(Ct), W, H, rX, rY, 7, 100, C.byref(prm), None, 0, 0, None, p(u32), p(u32, 4 * NP),
                                                 None, p(f64), None, None, st, None),
             lambda: lib.fsgm_sgm2d_device_exact(n, p(Ct), W, H, rX, rY, 7, 100, C.byref(prm), None, 0, 0, None, p(u32), p(u32, 4 * NP),
                                                 p(u32, 8 * NP), p(f64), None, None, st, None)]
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
        assert status == FSGM_ERR_UNSUPPORTED and "captured" in err
    assert bool((u32 == 0xABCD).all()) and bool((f64 == -7.0).all()), "a refused call queued something"
    assert [call() for call in calls] == [0, 0]                  # the same calls outside the capture run
    s.synchronize()
    assert not bool((u32 == 0xABCD).all()) and not bool((f64 == -7.0).all())
