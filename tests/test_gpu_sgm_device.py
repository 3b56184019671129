"""GPU tests of sgm(C) on caller-supplied cost volumes: the ingest kernel alone, then fsgm_sgm_batch_host, fsgm_sgm_device and
fsgm::sgm against the oracle's aggregation and WTA (pinned to the reference's compiled code), bit for bit.

The ingest kernel's tile is INGEST_TX x INGEST_TD = 64 pixels x 64 candidates (fsgm_amd/csrc/sgm_ingest.h), read 4 bytes a lane
along x and written 4 bytes a lane along d; the straight copy moves 16 bytes a lane, 4 KiB a workgroup.  The shapes below cross
1, 4, 16, tile - 1, tile, tile + 1 and two tiles + 3 in both directions."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, synth, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd.epi import EpiPlan  # noqa: E402
from fsgm_amd.sgm import _bind, last_kernel, params, sgm_batch  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import adaptive_p2_restatement as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_INVALID, FSGM_ERR_HIP = 1, 2
WIDTHS = (1, 31, 32, 33, 67, 63, 64, 65, 131)
DISPARITIES = (1, 15, 16, 17, 48, 63, 64, 65, 129)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _volumes(W, H, D, n, seed, cmax):
    """(n, H, W, D) uint8, every frame its own draw"""
    return np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])


def _as(layout, vols):
    return vols if layout == "hwd" else np.ascontiguousarray(vols.transpose(0, 3, 1, 2))


@functools.lru_cache(maxsize=None)
def _oracle_cached(key, P1, P2, paths):
    vols = _VOLS[key]
    out = []
    for Cv in vols:
        H, W, D = Cv.shape
        S = pyoracle.epi_aggregate(Cv, P1, P2, paths)
        out.append(pyoracle.epi_wta(S, W, H, D, 1) + (S[:-1].reshape(H, W, D),))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


_VOLS = {}


def _want(vols, P1, P2, paths):
    """(bestD, minC, S) of the oracle for every frame, computed once per distinct input"""
    key = (vols.shape, hash(vols.tobytes()))
    _VOLS.setdefault(key, vols)
    return _oracle_cached(key, P1, P2, paths)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("bestD", "minC", "S")):
        g = _n(g) if isinstance(g, torch.Tensor) else g
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


# ---------------------------------------------------------------------------------------------- 1. the ingest kernel alone
@pytest.mark.parametrize("D", DISPARITIES)
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
def test_ingest_alone(gpu_lib, layout, D):
    for W in WIDTHS:
        for H in (1, 5):
            for n in (1, 3):
                vols = _volumes(W, H, D, n, seed=W + 7 * H + D, cmax=255)
                with EpiPlan(W, H, D, n, vz_to_disp=0) as plan:
                    st = plan.ingest_cost(_t(_as(layout, vols)), layout=layout, cost_bound=255, return_status=True)
                    for f in range(n):
                        np.testing.assert_array_equal(plan.download_cost(f), vols[f], err_msg=f"{layout} {W}x{H}x{D} n={n} frame {f}")
                    assert int(st.item()) == 0


@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("W,H,D,n", [(67, 5, 129, 3), (33, 5, 17, 1), (64, 1, 64, 1), (131, 5, 48, 1)])
def test_ingest_from_an_odd_address(gpu_lib, layout, W, H, D, n):
    """u8 has no alignment rule: the source one byte into a larger allocation"""
    vols = _volumes(W, H, D, n, seed=5, cmax=255)
    src = _as(layout, vols)
    big = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    big[1:] = _t(src).reshape(-1)
    view = big[1:].view(src.shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    with EpiPlan(W, H, D, n, vz_to_disp=0) as plan:
        plan.ingest_cost(view, layout=layout, check=True)
        for f in range(n):
            np.testing.assert_array_equal(plan.download_cost(f), vols[f])


@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("W,H,D,n,bound", [(67, 5, 129, 3, 100), (65, 1, 17, 1, 1), (33, 5, 64, 1, 254), (1, 1, 1, 1, 127), (31, 5, 15, 3, 128)])
def test_ingest_saturates_at_the_bound(gpu_lib, layout, W, H, D, n, bound):
    vols = _volumes(W, H, D, n, seed=9, cmax=255)
    vols[-1, -1, -1, -1] = 255                                  # the last byte of the last frame is above every bound here
    with EpiPlan(W, H, D, n, vz_to_disp=0) as plan:
        st = plan.ingest_cost(_t(_as(layout, vols)), layout=layout, cost_bound=bound, return_status=True)
        for f in range(n):
            np.testing.assert_array_equal(plan.download_cost(f), np.minimum(vols[f], bound))
        assert int(st.item()) == FSGM_ERR_INVALID
        st = plan.ingest_cost(_t(_as(layout, np.minimum(vols, bound))), layout=layout, cost_bound=bound, return_status=True)
        assert int(st.item()) == 0                              # the flag was cleared, a clean volume raises none


# ---------------------------------------------------------------------------------------------- 2. the full call against the oracle
def _run(form, layout, vols, P1, P2, **kw):
    """(bestD, minC, S) of one of the three forms"""
    src = _as(layout, vols)
    if form == "host":
        return sgm_batch(src, P1, P2, layout=layout, return_sum=True, **kw)
    if form == "torch":
        return torch_ops.sgm(_t(src), P1, P2, layout=layout, return_sum=True, check=True, **kw)
    return _device_call(_t(src), layout, vols.shape, P1, P2, **kw)


def _device_call(Ct, layout, shape, P1, P2, *, paths=4, cost_bound=255, agg_mode=0, adaptive_p2=0, guide=None, want=0):
    """fsgm_sgm_device through ctypes on torch's current stream; asserts the status word"""
    lib = _bind(_lib.load())
    n, H, W, D = shape
    bestD, minC = (torch.empty((n, H, W), dtype=torch.uint32, device=DEV) for _ in range(2))
    S = torch.empty((n, H, W, D), dtype=torch.uint32, device=DEV)
    status = torch.full((), -1, dtype=torch.int32, device=DEV)
    prm = params(lib, paths=paths, device=0, agg_mode=agg_mode, layout=layout, cost_bound=cost_bound, adaptive_p2=adaptive_p2)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(lib.fsgm_sgm_device(n, p(Ct), W, H, D, P1, P2, C.byref(prm), p(guide), p(bestD), p(minC), p(S),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream), p(status)))
    torch.cuda.current_stream().synchronize()
    assert int(status.item()) == want
    return bestD, minC, S


@pytest.mark.parametrize("form", ["host", "device", "torch"])
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("W,H,D,n,kernel", [(33, 9, 16, 3, "packed16/wrap"), (67, 5, 48, 1, "packed16/wrap"), (20, 7, 20, 1, "generic")])
def test_full_call_against_the_oracle(gpu_lib, oracle, W, H, D, n, kernel, paths, layout, form):
    vols = _volumes(W, H, D, n, seed=3, cmax=255)
    got = _run(form, layout, vols, 7, 100, paths=paths)
    assert last_kernel() == kernel
    _same(got, _want(vols, 7, 100, paths), f"{form} {layout}")


@pytest.mark.parametrize("form", ["host", "device", "torch"])
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
def test_wrapping_penalties_with_the_full_bound(gpu_lib, oracle, layout, form):
    """cm + P2 + max(P1, P2) > 255: the wrapping line kernels, also for a volume whose costs happen to be small"""
    vols = _volumes(33, 9, 16, 3, seed=4, cmax=24)
    got = _run(form, layout, vols, 100, 200, paths=8, cost_bound=255)
    assert last_kernel() == "packed16/wrap"
    _same(got, _want(vols, 100, 200, 8), f"{form} {layout}")


def test_small_bound_selects_the_nowrap_kernels(gpu_lib, oracle):
    """the declared bound, not 255, is what the device form selects by"""
    vols = _volumes(33, 9, 16, 3, seed=4, cmax=24)
    got = _run("torch", "dhw", vols, 6, 32, paths=8, cost_bound=24)
    assert last_kernel() == "packed16/nowrap"
    _same(got, _want(vols, 6, 32, 8), "bound 24")
    got = _run("torch", "dhw", vols, 6, 32, paths=8, cost_bound=255)      # 255 + 32 + 32 > 255
    assert last_kernel() == "packed16/wrap"
    _same(got, _want(vols, 6, 32, 8), "bound 255")


# ---------------------------------------------------------------------------------------------- 3. every pipeline
MODES = [(2, 8, "sweep16/nowrap"), (2, 4, "pairs16/nowrap"), (3, 8, "sweep16par/nowrap"), (6, 8, "sweep16mid/nowrap"),
         (4, 8, "band16/nowrap"), (5, 8, "band16chain/nowrap")]


@pytest.mark.parametrize("mode,paths,kernel", MODES)
def test_every_pipeline_on_a_callers_volume(gpu_lib, oracle, mode, paths, kernel):
    vols = _volumes(40, 12, 16, 4, seed=6, cmax=24)
    Ct = _t(_as("dhw", vols))
    *got, status = torch_ops.sgm(Ct, 6, 32, layout="dhw", paths=paths, cost_bound=24, agg_mode=mode, return_sum=True, return_status=True)
    torch.cuda.synchronize()
    assert last_kernel() == kernel
    assert int(status.item()) == 0, "FSGM_ERR_HIP here is a hand-off that gave up: a finding, not something to retry"
    _same(got, _want(vols, 6, 32, paths), f"mode {mode}")
    lines = torch_ops.sgm(Ct, 6, 32, layout="dhw", paths=paths, cost_bound=24, agg_mode=1, return_sum=True, check=True)
    assert last_kernel() == "packed16/nowrap"
    for g, l in zip(got, lines):
        assert torch.equal(g, l)


# ---------------------------------------------------------------------------------------------- 4. the bound
def test_the_bound(gpu_lib, oracle):
    W, H, D, n = 33, 9, 16, 3
    clean = _volumes(W, H, D, n, seed=8, cmax=24)
    vols = clean.copy()
    vols[0, 0, 0, 0] = vols[1, 4, 17, 9] = vols[2, H - 1, W - 1, D - 1] = 200
    for layout in ("hwd", "dhw"):
        Ct = _t(_as(layout, vols))
        *got, st = torch_ops.sgm(Ct, 6, 32, layout=layout, paths=8, cost_bound=24, return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == FSGM_ERR_INVALID and last_kernel() == "packed16/nowrap"
        _same(got, _want(np.minimum(vols, 24), 6, 32, 8), f"saturated {layout}")
        with pytest.raises(FsgmError) as e:
            torch_ops.sgm(Ct, 6, 32, layout=layout, paths=8, cost_bound=24, check=True)
        assert e.value.status == FSGM_ERR_INVALID
        with pytest.raises(FsgmError) as e:
            sgm_batch(_as(layout, vols), 6, 32, layout=layout, paths=8, cost_bound=24)
        assert e.value.status == FSGM_ERR_INVALID
        *got, st = torch_ops.sgm(Ct, 6, 32, layout=layout, paths=8, cost_bound=255, return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        _same(got, _want(vols, 6, 32, 8), f"bound 255 {layout}")
        _same(sgm_batch(_as(layout, vols), 6, 32, layout=layout, paths=8, return_sum=True), _want(vols, 6, 32, 8), f"host 255 {layout}")
        *got, st = torch_ops.sgm(_t(_as(layout, clean)), 6, 32, layout=layout, paths=8, cost_bound=24, return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        _same(got, _want(clean, 6, 32, 8), f"clean {layout}")


def test_the_bound_flag_is_cleared_by_the_call_that_reports_it(gpu_lib):
    """one cost above the bound: FSGM_ERR_INVALID, and 0 from the very next call at the same shape on the same stream"""
    N, D, H, W = 2, 16, 5, 7
    clean = _as("dhw", _volumes(W, H, D, N, seed=12, cmax=32))
    over = clean.copy()
    over[1, 9, 3, 4] = 200
    status = [torch_ops.sgm(_t(v), 6, 32, layout="dhw", cost_bound=32, return_status=True)[-1] for v in (over, clean)]
    torch.cuda.synchronize()
    assert [int(s.item()) for s in status] == [FSGM_ERR_INVALID, 0]


# ---------------------------------------------------------------------------------------------- 5. adaptive P2
@pytest.mark.parametrize("paths", [4, 8])
def test_adaptive_p2(gpu_lib, paths):
    W, H, D, n = 33, 9, 16, 3
    vols = _volumes(W, H, D, n, seed=10, cmax=24)
    guide = np.stack([synth.image_pair(W, H, D, seed=20 + f)[0] for f in range(n)])
    guide[:, :, W // 2:] = np.minimum(guide[:, :, W // 2:].astype(np.int32) + 120, 255).astype(np.uint8)      # a step edge
    want = []
    for f in range(n):
        S = A.aggregate(vols[f], guide[f], 6, 64, paths, adaptive=1)
        want.append(pyoracle.epi_wta(S, W, H, D, 1) + (S[:-1].reshape(H, W, D),))
    want = tuple(np.stack([w[k] for w in want]) for k in range(3))
    plain = _want(vols, 6, 64, paths)
    assert not np.array_equal(want[0], plain[0]) or not np.array_equal(want[2], plain[2]), "the edge must matter"
    for layout in ("hwd", "dhw"):
        src = _as(layout, vols)
        _same(sgm_batch(src, 6, 64, layout=layout, paths=paths, adaptive_p2=1, guide=guide, return_sum=True), want, f"host {layout}")
        _same(torch_ops.sgm(_t(src), 6, 64, layout=layout, paths=paths, adaptive_p2=1, guide=_t(guide), return_sum=True, check=True),
              want, f"torch {layout}")
        _same(_device_call(_t(src), layout, vols.shape, 6, 64, paths=paths, adaptive_p2=1, guide=_t(guide)), want, f"device {layout}")
    for call in (lambda: sgm_batch(vols, 6, 64, adaptive_p2=1), lambda: torch_ops.sgm(_t(vols), 6, 64, layout="hwd", adaptive_p2=1)):
        with pytest.raises(FsgmError) as e:
            call()
        assert e.value.status == FSGM_ERR_INVALID


# ---------------------------------------------------------------------------------------------- 6. stream order
def test_stream_order_on_a_side_stream(gpu_lib, oracle):
    """C filled by a torch kernel on a side stream just before the call on that stream, no synchronisation in between"""
    W, H, D, n = 160, 96, 64, 2
    vols = _volumes(W, H, D, n, seed=11, cmax=24)
    host = torch.from_numpy(_as("dhw", vols)).pin_memory()
    ref = torch_ops.sgm(_t(_as("dhw", vols)), 6, 32, paths=8, cost_bound=24, check=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Ct = torch.zeros((n, D, H, W), dtype=torch.uint8, device=DEV)
        up = host.to(DEV, non_blocking=True)
        Ct.copy_((up.to(torch.int16) + 0).to(torch.uint8))          # filled by kernels on s
        bd, mc = torch_ops.sgm(Ct, 6, 32, paths=8, cost_bound=24)
        bd2 = bd.clone()
        Ct.zero_()                                                  # queued after the call: must not reach it
    s.synchronize()
    assert torch.equal(bd2, ref[0]) and torch.equal(mc, ref[1])
    _same((bd2, mc), _want(vols, 6, 32, 8)[:2], "side stream")


# ---------------------------------------------------------------------------------------------- 7. pointer checks
def test_pointer_checks(gpu_lib):
    lib = _bind(_lib.load())
    W, H, D, n = 33, 9, 16, 3
    NP, N = W * H, W * H * D
    Ct = torch.zeros(n * N, dtype=torch.uint8, device=DEV)
    out = torch.full((2 * n * NP + 1,), 0xABCD, dtype=torch.int32, device=DEV)
    bestD, minC = out.data_ptr(), out.data_ptr() + 4 * n * NP
    pinned = torch.zeros(n * N, dtype=torch.uint8).pin_memory()
    prm = lib.fsgm_sgm_params_default()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda Cp, bd: lib.fsgm_sgm_device(n, C.c_void_p(Cp), W, H, D, 7, 100, C.byref(prm), None, C.c_void_p(bd),  # noqa: E731
                                              C.c_void_p(minC), None, stream, None)
    err = lambda: lib.fsgm_last_error().decode()  # noqa: E731
    assert call(pinned.data_ptr(), bestD) == FSGM_ERR_INVALID and "not device memory" in err()
    # one frame short: an allocation of its own, straight from the runtime (torch's allocator hands out parts of larger ones)
    hip = C.CDLL(torch_ops.hip_runtimes()[0])
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), (n - 1) * N) == 0
    try:
        assert call(short.value, bestD) == FSGM_ERR_INVALID and "its allocation holds" in err()
    finally:
        hip.hipFree(short)
    assert call(Ct.data_ptr(), bestD + 2) == FSGM_ERR_INVALID and "not aligned" in err()
    torch.cuda.synchronize()
    assert bool((out == 0xABCD).all()), "a refused call queued something"
    assert call(Ct.data_ptr(), bestD) == 0
    torch.cuda.synchronize()
    assert not bool((out[:2 * n * NP] == 0xABCD).all())
