"""GPU tests of fsgm::sgm_exact (torch_ops.sgm(arith="exact"), fsgm_sgm_device_exact): tensors in HBM in and out on the caller's
stream, against the host form (fsgm_amd.sgm_batch(arith="exact")) and its yardstick tests/sgm_exact_restatement.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd.sgm import last_kernel, sgm_batch  # noqa: E402
from tests import sgm_exact_restatement as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _dhw(vols):
    return np.ascontiguousarray(vols.transpose(0, 3, 1, 2))


def _vols(W, H, D, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, D), dtype=np.uint8)


@pytest.mark.parametrize("W,H,D,n,paths", [(37, 11, 64, 3, 8), (9, 21, 48, 1, 4), (37, 11, 300, 2, 8), (9, 21, 256, 3, 4)])
def test_op_equals_the_host_form(gpu_lib, W, H, D, n, paths):
    vols = _vols(W, H, D, n, D + n)
    host = sgm_batch(vols, 7, 100, paths=paths, arith="exact", return_sum=True)
    want = X.sgm_batch(vols, 7, 100, paths)
    bd, mc, S, st = torch_ops.sgm(_t(_dhw(vols)), 7, 100, paths=paths, arith="exact", return_sum=True, return_status=True)
    assert last_kernel() == ("generic/exact" if D == 300 else "packed16/exact")
    assert S.is_cuda and S.dtype == torch.uint32 and tuple(S.shape) == (n, H, W, D) and int(st.item()) == 0
    for g, h, w, name in zip((bd, mc, S), host, want, ("bestD", "minC", "S")):
        assert np.array_equal(_n(g), h), f"{name}: op against the host form"
        assert np.array_equal(h, w), f"{name}: host form against the restatement"
    # one volume without the batch dimension, the other layout, no S
    bd1, mc1 = torch_ops.sgm(_t(vols[0]), 7, 100, paths=paths, layout="hwd", arith="exact", check=True)
    assert np.array_equal(_n(bd1), want[0][0]) and np.array_equal(_n(mc1), want[1][0])
    # the plain op on the same tensor is still the mod-256 rule
    pbd, _ = torch_ops.sgm(_t(_dhw(vols)), 7, 100, paths=paths)
    assert last_kernel() in ("packed16/wrap", "generic") and not np.array_equal(_n(pbd), want[0])


def test_adaptive_p2_and_a_bound_below_the_costs(gpu_lib):
    W, H, D, n = 37, 11, 32, 2
    vols = _vols(W, H, D, n, 5)
    guides = np.random.default_rng(6).choice(np.array([10, 30, 40, 70, 200], np.uint8), (n, H, W))
    bd, mc, S = torch_ops.sgm(_t(_dhw(vols)), 7, 100, paths=8, arith="exact", adaptive_p2=1, guide=_t(guides), return_sum=True)
    for g, w in zip((bd, mc, S), X.sgm_batch(vols, 7, 100, 8, guides)):
        assert np.array_equal(_n(g), w)
    # cost_bound as in fsgm::sgm: the ingest saturates at it and the status word says so
    bd, mc, st = torch_ops.sgm(_t(_dhw(vols)), 7, 100, paths=8, arith="exact", cost_bound=99, return_status=True)
    assert int(st.item()) == torch_ops.FSGM_ERR_INVALID
    for g, w in zip((bd, mc), X.sgm_batch(np.minimum(vols, 99), 7, 100, 8)):
        assert np.array_equal(_n(g), w)


def test_on_a_side_stream(gpu_lib):
    """the volume filled by kernels on a side stream just before the call on that stream, and cleared right after it"""
    W, H, D, n = 37, 11, 128, 3
    vols = _vols(W, H, D, n, 8)
    want = X.sgm_batch(vols, 0, 255, 8)
    host = torch.from_numpy(_dhw(vols)).pin_memory()
    torch_ops.sgm(_t(_dhw(vols)), 0, 255, paths=8, arith="exact", check=True)         # the shape is warm
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Ct = torch.zeros((n, D, H, W), dtype=torch.uint8, device=DEV)
        Ct.copy_((host.to(DEV, non_blocking=True).to(torch.int16) + 0).to(torch.uint8))
        bd, mc, S = torch_ops.sgm(Ct, 0, 255, paths=8, arith="exact", return_sum=True)
        bd2 = bd.clone()
        Ct.zero_()                                               # queued after the call: must not reach it
    s.synchronize()
    assert np.array_equal(_n(bd2), want[0]) and np.array_equal(_n(mc), want[1]) and np.array_equal(_n(S), want[2])


def test_graph_capture_and_replay(gpu_lib):
    """a warm shape queues work and nothing else: captured once, replayed on new contents of the same tensors"""
    W, H, D, n = 37, 11, 64, 2
    a, b = _vols(W, H, D, n, 21), _vols(W, H, D, n, 22)
    Ct = _t(_dhw(a))
    torch_ops.sgm(Ct, 7, 100, paths=8, arith="exact", return_sum=True, check=True)     # warm: plan, buffers, S tap
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bd, mc, S, st = torch_ops.sgm(Ct, 7, 100, paths=8, arith="exact", return_sum=True, return_status=True)
    for vols in (a, b, a):
        Ct.copy_(_t(_dhw(vols)))
        g.replay()
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        for got, w in zip((bd, mc, S), X.sgm_batch(vols, 7, 100, 8)):
            assert np.array_equal(_n(got), w)
    # and the shape still serves eager calls
    bd2, mc2 = torch_ops.sgm(_t(_dhw(b)), 7, 100, paths=8, arith="exact", check=True)
    assert np.array_equal(_n(bd2), X.sgm_batch(b, 7, 100, 8)[0])


def test_a_captured_call_needs_a_warm_plan(gpu_lib):
    """a capture may allocate nothing: a shape that never ran, and a warm shape asked for S for the first time, are refused with
    status 4 before anything is queued; the same calls run outside the capture"""
    from fsgm_amd._lib import FsgmError
    W, H, D, n = 9, 21, 80, 2                                    # a shape no other test of this file uses
    vols = _vols(W, H, D, n, 31)
    Ct = _t(_dhw(vols))
    want = X.sgm_batch(vols, 7, 100, 4)
    for warm_up, kw in ((None, {}), ({}, {"return_sum": True})):
        if warm_up is not None:
            torch_ops.sgm(Ct, 7, 100, paths=4, arith="exact", check=True, **warm_up)
        torch.cuda.synchronize()
        with pytest.raises(FsgmError) as ei:
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                torch_ops.sgm(Ct, 7, 100, paths=4, arith="exact", **kw)
        assert ei.value.status == 4 and "captured" in str(ei.value)
        torch.cuda.synchronize()
    bd, mc, S = torch_ops.sgm(Ct, 7, 100, paths=4, arith="exact", return_sum=True, check=True)
    for got, w in zip((bd, mc, S), want):
        assert np.array_equal(_n(got), w)


def test_a_captured_plan_outlives_the_plan_cache(gpu_lib):
    """the graph names the cached plan's buffers: six other cold shapes go through the cache of four plans, exact and plain, and
    the replay still computes -- the recorded plan is pinned, not evicted"""
    W, H, D, n = 37, 11, 96, 2
    a, b = _vols(W, H, D, n, 41), _vols(W, H, D, n, 42)
    Ct = _t(_dhw(a))
    torch_ops.sgm(Ct, 7, 100, paths=8, arith="exact", check=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bd, mc = torch_ops.sgm(Ct, 7, 100, paths=8, arith="exact")
    for k, d in enumerate((16, 32, 48, 64, 112, 24)):            # plans of other shapes, some of them large enough to reuse freed memory
        other = _vols(61 + k, 40, d, 3, d)
        torch_ops.sgm(_t(_dhw(other)), 7, 100, paths=8, arith="exact" if k % 2 else "mod256", check=True)
    for vols in (b, a):
        Ct.copy_(_t(_dhw(vols)))
        g.replay()
        torch.cuda.synchronize()
        want = X.sgm_batch(vols, 7, 100, 8)
        assert np.array_equal(_n(bd), want[0]) and np.array_equal(_n(mc), want[1])
    # an eager call of the recorded shape on the replay's stream is ordered behind it by the event join
    Ct.copy_(_t(_dhw(a)))
    g.replay()
    bd2, mc2 = torch_ops.sgm(_t(_dhw(b)), 7, 100, paths=8, arith="exact")
    first = bd.clone()
    torch.cuda.synchronize()
    assert np.array_equal(_n(first), X.sgm_batch(a, 7, 100, 8)[0]) and np.array_equal(_n(bd2), X.sgm_batch(b, 7, 100, 8)[0])


def test_exact_with_runner_up_raises(gpu_lib):
    with pytest.raises(ValueError, match="runner"):
        torch_ops.sgm(_t(_dhw(_vols(9, 21, 16, 1, 1))), arith="exact", runner_up=True)
