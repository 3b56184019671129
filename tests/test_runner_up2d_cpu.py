"""CPU tests of the 2-D matcher's runner-up cost: the numpy restatement against a plain triple loop, its 1-D special case, every
refusal of the new entry points that answers before a device is touched, and the new torch ops' schemas and fake implementations."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, pyd as _pyd, sgm2d as _sgm2d  # noqa: E402
from tests import runner_up_restatement as RU  # noqa: E402
from tests import runner_up2d_restatement as RU2  # noqa: E402

_sgm = importlib.import_module("fsgm_amd.sgm")   # (the name fsgm_amd.sgm is the function sgm(C, P1, P2), not this submodule)

INVALID, UNSUPPORTED = 1, 4
NONE = RU.NO_RUNNER_UP
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first
WINDOWS = [(1, 1), (3, 3), (3, 1), (5, 1), (1, 5), (5, 3)]


def _loop(S, Sx, Sy):
    """the definition as a triple loop over pixels, sx and sy"""
    S = np.asarray(S).reshape(-1, Sx * Sy)
    best, minC, minC2 = [], [], []
    for row in S:
        b, lo = 0, int(row[0])
        for d in range(1, Sx * Sy):
            if int(row[d]) < lo:
                b, lo = d, int(row[d])
        bx, by = divmod(b, Sy)
        c2 = NONE
        for sx in range(Sx):
            for sy in range(Sy):
                if max(abs(sx - bx), abs(sy - by)) >= 2:
                    c2 = min(c2, int(row[sx * Sy + sy]))
        best.append(b), minC.append(lo), minC2.append(c2)
    return np.array(best), np.array(minC, np.uint32), np.array(minC2, np.uint32)


@pytest.mark.parametrize("Sx,Sy", WINDOWS)
def test_restatement_equals_the_triple_loop(Sx, Sy):
    rng = np.random.default_rng(10 * Sx + Sy)
    for hi in (4, 2041, 2 ** 32 - 1):                            # dense ties; the u16 range; sums up to the marker's neighbourhood
        S = rng.integers(0, hi, (6, 7, Sx * Sy), dtype=np.uint64).astype(np.uint32)
        S[0, 0] = 5                                              # constant: best 0
        for k, d in enumerate(range(Sx * Sy)):                   # the minimum at every candidate in turn
            S[1 + k // 7 % 5, k % 7, d] = 0
        got = RU2.runner_up2d(S, Sx, Sy)
        want = _loop(S, Sx, Sy)
        for g, w, name in zip(got, want, ("best", "minC", "minC2")):
            np.testing.assert_array_equal(np.asarray(g).ravel(), w, err_msg=f"{Sx}x{Sy} {name}")
        assert got[1].dtype == np.uint32 and got[2].dtype == np.uint32


def test_where_the_set_is_empty():
    for Sx, Sy in ((1, 1), (2, 2), (1, 2), (2, 1)):
        assert (RU2.runner_up2d(np.arange(Sx * Sy, dtype=np.uint32)[::-1].copy(), Sx, Sy)[2] == NONE)
    S = np.full(9, 7, np.uint32)
    S[4] = 1                                                     # 3x3, best in the middle: all eight others are the ring
    assert RU2.runner_up2d(S, 3, 3) == (4, 1, NONE)
    S[4], S[0] = 7, 1                                            # best in a corner: the far row and column compete
    assert RU2.runner_up2d(S, 3, 3) == (0, 1, 7)
    S = np.array([9, 1, 9], np.uint32)
    assert RU2.runner_up2d(S, 3, 1)[2] == NONE and RU2.runner_up2d(S, 1, 3)[2] == NONE
    S = np.full(15, 9, np.uint32)
    S[7] = 0                                                     # 5x3, best (2, 1): columns 0 and 4 are two away
    S[6], S[3], S[1] = 1, 2, 3                                   # (2, 0) and (1, 0) in the ring, (0, 1) outside it
    assert RU2.runner_up2d(S, 5, 3) == (7, 0, 3)


def test_one_row_of_candidates_is_the_1d_rule():
    rng = np.random.default_rng(3)
    for D in (1, 2, 3, 5, 16, 63):
        S = rng.integers(0, 6, (40, D)).astype(np.uint32)
        for a, b in zip(RU2.runner_up2d(S, D, 1), RU.runner_up(S)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(RU2.runner_up2d(S, 1, D), RU.runner_up(S)):
            np.testing.assert_array_equal(a, b)


def test_flow_filter_restatement():
    flow = np.arange(2 * 2 * 3, dtype=np.float64).reshape(2, 2, 3)
    flow[1, 0, 0] = np.nan
    c = np.uint32([[10, 10, 0], [10, 10, 10]])
    c2 = np.uint32([[10, 99, 0], [NONE, 11, 12]])
    out = RU2.uniqueness_filter_flow(flow, c, c2, 15)
    rej = np.array([[True, False, False], [False, True, False]])
    assert np.isnan(out[:, rej]).all() and np.isnan(out[1, 0, 0])
    keep = ~rej
    keep[0, 0] = False
    np.testing.assert_array_equal(out[0][keep], flow[0][keep])


# ---- refusals before a device ----
def _err(lib):
    return lib.fsgm_last_error().decode()


def test_sgm2d_ru_entry_points_refuse_before_any_device():
    lib = _sgm2d._bind(_lib.load())
    host = lambda n=1, W=8, H=4, rX=1, rY=1, m2=FAKE, prm=None: lib.fsgm_sgm2d_batch_host_ru(                     # noqa: E731
        n, FAKE, W, H, rX, rY, 6, 32, prm, None, 0, 0, None, FAKE, FAKE, m2, FAKE, None, None)
    dev = lambda n=1, W=8, H=4, rX=1, rY=1, m2=FAKE, prm=None: lib.fsgm_sgm2d_device_ru(                          # noqa: E731
        n, FAKE, W, H, rX, rY, 6, 32, prm, None, 0, 0, None, FAKE, FAKE, m2, FAKE, None, None, None, None)
    for fn in (host, dev):
        assert fn(m2=None) == INVALID and "minC2" in _err(lib)
        assert fn(n=0) == INVALID and "n_frames" in _err(lib)
        assert fn(W=0) == INVALID and "width/height" in _err(lib)
        assert fn(rX=-1) == INVALID
        assert fn(rX=32) == UNSUPPORTED and fn(rX=16, rY=16) == UNSUPPORTED
        bad = _sgm2d.params(lib)
        bad.cost_bound = 0
        assert fn(prm=C.byref(bad)) == INVALID and "cost_bound" in _err(lib)


def test_sgm_ru_entry_points_refuse_before_any_device():
    lib = _sgm._bind(_lib.load())
    host = lambda n=1, W=8, H=4, D=16, m2=FAKE, prm=None: lib.fsgm_sgm_batch_host_ru(                            # noqa: E731
        n, FAKE, W, H, D, 7, 100, prm, None, FAKE, FAKE, m2, None)
    dev = lambda n=1, W=8, H=4, D=16, m2=FAKE, prm=None: lib.fsgm_sgm_device_ru(                                 # noqa: E731
        n, FAKE, W, H, D, 7, 100, prm, None, FAKE, FAKE, m2, None, None, None)
    for fn in (host, dev):
        assert fn(m2=None) == INVALID and "minC2" in _err(lib)
        assert fn(n=0) == INVALID and fn(W=0) == INVALID and fn(D=1025) == INVALID
        for mode in (2, 3, 4, 5, 6):
            prm = _sgm.params(lib, agg_mode=mode)
            assert fn(prm=C.byref(prm)) == UNSUPPORTED and "runner-up" in _err(lib) and f"agg_mode {mode}" in _err(lib)
        prm = _sgm.params(lib, agg_mode=7)
        assert fn(prm=C.byref(prm)) == INVALID
    # the plain forms still take the forced modes as far as their own checks go (a NULL C stops them here)
    prm = _sgm.params(lib, agg_mode=4)
    assert lib.fsgm_sgm_batch_host(1, None, 8, 4, 16, 7, 100, C.byref(prm), None, FAKE, FAKE, None) == INVALID and "null" in _err(lib)


def test_pyd_ru_entry_points_refuse_before_any_device():
    lib = _lib.load()
    _pyd._bind(lib)
    assert lib.fsgm_pyd_plan_set_runner_up(None, 1) == INVALID and "null plan" in _err(lib)
    assert lib.fsgm_pyd_plan_download_runner_up(None, 0, FAKE) == INVALID and "null" in _err(lib)
    a, o = _pyd.PydIn(), _pyd.PydOut()
    assert lib.fsgm_calc_pyd_cost_sgm_batch_host_ru(1, C.byref(a), C.byref(o), None, 0) == INVALID and "minC2s" in _err(lib)
    none = (C.c_void_p * 1)(None)
    assert lib.fsgm_calc_pyd_cost_sgm_batch_host_ru(1, C.byref(a), C.byref(o), none, 0) == INVALID and "minC2" in _err(lib)
    some = (C.c_void_p * 1)(FAKE)
    assert lib.fsgm_calc_pyd_cost_sgm_batch_host_ru(0, C.byref(a), C.byref(o), some, 0) == INVALID
    assert lib.fsgm_calc_pyd_cost_sgm_batch_host_ru(1, C.byref(a), C.byref(o), some, 0) == INVALID and "null input" in _err(lib)


def test_filter_planes_refuses_before_any_device():
    lib = _lib.load()
    m = np.zeros((2, 2, 4, 6))
    c, c2 = np.zeros((2, 4, 6), np.uint32), np.zeros((2, 4, 6), np.uint32)
    p = _lib.ptr
    host = lambda n=2, W=6, H=4, planes=2, ratio=15, a=p(m), b=p(c), d=p(c2), o=p(m), device=0: (                # noqa: E731
        lib.fsgm_uniqueness_filter_planes_host(n, a, b, d, W, H, planes, ratio, o, device))
    dev = lambda n=2, W=6, H=4, planes=2, ratio=15, a=p(m), b=p(c), d=p(c2), o=p(m), device=0: (                 # noqa: E731
        lib.fsgm_uniqueness_filter_planes_device(n, a, b, d, W, H, planes, ratio, o, device, None, None))
    for fn in (host, dev):
        for planes in (0, 3, -1):
            assert fn(planes=planes) == INVALID and "planes" in _err(lib)
        for ratio in (-1, 101):
            assert fn(ratio=ratio) == INVALID and "ratio" in _err(lib)
        for k in ("a", "b", "d", "o"):
            assert fn(**{k: None}) == INVALID and "null" in _err(lib)
        assert fn(n=0) == INVALID and fn(W=0) == INVALID and fn(H=0) == INVALID
        assert fn(o=p(c)) == INVALID and "overlap" in _err(lib)
        assert fn(o=p(c2)) == INVALID and "overlap" in _err(lib)
        assert fn(o=C.c_void_p(m.ctypes.data + 8)) == INVALID and "map itself" in _err(lib)
        # the second plane is part of the array: an out that starts inside it overlaps with planes = 2 ...
        assert fn(o=C.c_void_p(m.ctypes.data + m.nbytes - 8)) == INVALID and "map itself" in _err(lib)
        assert fn(device=64) == INVALID and "out of range" in _err(lib)
    assert not m.any()


def test_python_wrappers_validate_before_the_library():
    m, f = np.zeros((4, 6)), np.zeros((2, 4, 6))
    c = np.zeros((4, 6), np.uint32)
    for planes in (0, 3, True, "2"):
        with pytest.raises(ValueError, match="planes"):
            fsgm_amd.uniqueness_filter(m, c, c, 5, planes=planes)
    with pytest.raises(TypeError, match="flow"):
        fsgm_amd.uniqueness_filter(m, c, c, 5, planes=2)
    with pytest.raises(TypeError, match="flow"):
        fsgm_amd.uniqueness_filter(np.zeros((3, 4, 6)), c, c, 5, planes=2)
    with pytest.raises(TypeError, match="minC"):
        fsgm_amd.uniqueness_filter(f, np.zeros((2, 4, 6), np.uint32), c, 5, planes=2)
    with pytest.raises(ValueError, match="ratio"):
        fsgm_amd.uniqueness_filter(f, c, c, 101, planes=2)
    for fn in (fsgm_amd.calc_pyd_cost_sgm, fsgm_amd.calc_pyd_cost_sgm_batch, fsgm_amd.sgm2d_batch, fsgm_amd.sgm_batch,
               torch_ops.sgm2d, torch_ops.sgm):
        assert inspect.signature(fn).parameters["runner_up"].default is False
    assert inspect.signature(fsgm_amd.uniqueness_filter).parameters["planes"].default == 1
    assert inspect.signature(torch_ops.uniqueness_filter).parameters["planes"].default == 1
    assert callable(fsgm_amd.PydPlan.set_runner_up) and callable(fsgm_amd.PydPlan.download_runner_up)


# ---- the torch ops ----
def test_schemas():
    assert str(torch.ops.fsgm.sgm_ru.default._schema) == (
        "fsgm::sgm_ru(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, "
        "SymInt adaptive_p2, SymInt subpixel, SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.sgm2d_ru.default._schema) == (
        "fsgm::sgm2d_ru(Tensor C_, Tensor hints, Tensor guide, SymInt half_x, SymInt half_y, SymInt P1, SymInt P2, SymInt layout, "
        "SymInt cost_bound, SymInt diagonal, SymInt total_pass, SymInt adaptive_p2, SymInt subpixel, SymInt return_flow, "
        "SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.uniqueness_filter_planes.default._schema) == (
        "fsgm::uniqueness_filter_planes(Tensor map_, Tensor minC, Tensor minC2, SymInt ratio, SymInt planes) -> (Tensor, Tensor)")
    # the neighbours are what they were
    assert str(torch.ops.fsgm.sgm.default._schema) == (
        "fsgm::sgm(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, "
        "SymInt adaptive_p2, SymInt subpixel, SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.sgm2d.default._schema) == (
        "fsgm::sgm2d(Tensor C_, Tensor hints, Tensor guide, SymInt half_x, SymInt half_y, SymInt P1, SymInt P2, SymInt layout, "
        "SymInt cost_bound, SymInt diagonal, SymInt total_pass, SymInt adaptive_p2, SymInt subpixel, SymInt return_flow, "
        "SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.uniqueness_filter.default._schema) == (
        "fsgm::uniqueness_filter(Tensor map_, Tensor minC, Tensor minC2, SymInt ratio) -> (Tensor, Tensor)")


def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    meta = lambda ts: [(tuple(t.shape), t.dtype, t.device.type) for t in ts]          # noqa: E731
    with FakeTensorMode():
        for lead in ((), (3,)):
            px = lead + (10, 21)
            costs = torch.empty(lead + (81, 10, 21), dtype=torch.uint8, device="cuda")
            r = torch_ops.sgm2d(costs, 4, 4, runner_up=True, return_flow=True, return_sum=True, return_status=True)
            assert meta(r) == [(px, torch.uint32, "cuda")] * 3 + [(lead + (2, 10, 21), torch.float64, "cuda")] * 2 + [
                (px + (81,), torch.uint32, "cuda"), ((), torch.int32, "cuda")]
            assert len(torch_ops.sgm2d(costs, 4, 4)) == 3 and len(torch_ops.sgm2d(costs, 4, 4, runner_up=True)) == 4
            vol = torch.empty(lead + (16, 10, 21), dtype=torch.uint8, device="cuda")
            r = torch_ops.sgm(vol, runner_up=True, return_sum=True)
            assert meta(r) == [(px, torch.uint32, "cuda")] * 3 + [(px + (16,), torch.uint32, "cuda")]
            assert len(torch_ops.sgm(vol)) == 2
            flow = torch.empty(lead + (2, 10, 21), dtype=torch.float64, device="cuda")
            c = torch.empty(px, dtype=torch.uint32, device="cuda")
            assert meta([torch_ops.uniqueness_filter(flow, c, c, 15, planes=2)]) == [(lead + (2, 10, 21), torch.float64, "cuda")]
            with pytest.raises(TypeError, match="shape"):
                torch_ops.uniqueness_filter(flow, torch.empty(lead + (2, 10, 21), dtype=torch.uint32, device="cuda"), c, 15, planes=2)
            with pytest.raises(ValueError, match="planes"):
                torch_ops.uniqueness_filter(flow, c, c, 15, planes=3)
            with pytest.raises(TypeError, match="planes=2"):
                torch_ops.uniqueness_filter(torch.empty((10, 21), dtype=torch.float64, device="cuda"), c, c, 15, planes=2)


def test_raw_filter_op_checks_its_shapes_in_the_fake_too():
    """fsgm::uniqueness_filter_planes sizes out from map_ and indexes N * planes * H * W elements: a map without `planes` planes
    is refused by the op itself, not only by the wrapper"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        m = torch.empty((2, 10, 21), dtype=torch.float64, device="cuda")
        f = torch.empty((2, 2, 10, 21), dtype=torch.float64, device="cuda")
        c = torch.empty((2, 10, 21), dtype=torch.uint32, device="cuda")
        for map_, planes in ((m, 2), (f, 1), (f[:, :, :5], 2)):
            with pytest.raises(TypeError, match="map_ must be"):
                torch.ops.fsgm.uniqueness_filter_planes(map_, c, c, 15, planes)
        with pytest.raises(TypeError, match="one shape"):
            torch.ops.fsgm.uniqueness_filter_planes(f, c, c[:1], 15, 2)
        with pytest.raises(ValueError, match="planes"):
            torch.ops.fsgm.uniqueness_filter_planes(f, c, c, 15, 0)
        out, st = torch.ops.fsgm.uniqueness_filter_planes(f, c, c, 15, 2)
        assert tuple(out.shape) == (2, 2, 10, 21) and tuple(st.shape) == ()
