"""The second view without a GPU (include/fsgm.h, "Second view"): the numpy restatement against a brute-force triple loop, the
planted volume, every refusal of the new entries before a device is touched (none is present here, so a status other than 2 proves
it), the LDS request at every dMax, and the existing wrappers' routing with the switch off."""
import ctypes as C
import itertools

import numpy as np
import pytest

try:                                                             # (before the library: torch_ops needs one HIP runtime in the process)
    import torch  # noqa: F401
except ImportError:
    torch = None

import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, view2
from fsgm_amd.sgm import SgmParams, _bind as _bind_sgm, params as sgm_params
from tests import view2_restatement as R

INVALID, UNSUPPORTED = 1, 4


# ---- the restatement ----
@pytest.mark.parametrize("direction,d_min,subpixel", list(itertools.product((-1, 1), (-3, 0, 5), (0, 1))))
def test_restatement_equals_the_triple_loop(direction, d_min, subpixel):
    rng = np.random.default_rng(100 + 7 * d_min + direction + subpixel)
    for H, W, D in ((2, 9, 4), (1, 5, 12), (3, 17, 8), (1, 1, 3)):          # (W < D among them)
        S = rng.integers(0, 4, (H, W, D)).astype(np.uint32) * 5              # few distinct values: ties
        d2, mc = R.view2(S, direction, d_min, subpixel)
        bd2, bmc = R.brute(S, direction, d_min, subpixel)
        assert np.array_equal(d2, bd2) and np.array_equal(mc, bmc)
        if subpixel == 0:
            assert ((d2 % 256 == 0) | (d2 == R.NO_VIEW2)).all()
    S = rng.integers(0, 4, (2, 2, 9, 4)).astype(np.uint32)                   # leading batch dimensions
    d2, mc = R.view2(S, direction, d_min, subpixel)
    assert np.array_equal(d2[1, 0], R.brute(S[1, 0][None], direction, d_min, subpixel)[0][0])


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("d_min", [-3, 0, 5])
def test_planted_volume(direction, d_min):
    H, W, D, k = 2, 30, 12, 4
    S = np.full((H, W, D), 20, np.uint32)
    S[..., k] = 0
    d2, mc = R.view2(S, direction, d_min, 1)
    x2 = np.arange(W)
    x = x2 - direction * (d_min + k)
    planted = (x >= 0) & (x < W)
    assert (d2[:, planted] == 256 * k).all() and (mc[:, planted] == 0).all()
    bestD = np.full((H, W), 256 * k, np.uint32)
    conf = R.check_sgm(bestD, d2, direction, d_min, 0)
    tgt = np.arange(W) + direction * (d_min + k)                             # where the first view's match lands
    assert np.array_equal(conf[0] == 1, (tgt >= 0) & (tgt < W))


def test_check_arithmetic():
    d1 = np.array([[-300, 127, 128, 100000]], np.int32)                      # (d1 + 128) >> 8: -1, 0, 1, 391 (arithmetic shift)
    d2 = np.array([[-300 + 256, 127, R.INT32_MIN, 0]], np.int32)
    assert R.check_true(d1, d2, -1, 256).tolist() == [[0, 1, 1, 0]]          # x2 = 1, 1, 1, out of range; |d1 - 127| = 427, 0, 1
    assert R.check_true(d1, d2, 1, 0).tolist() == [[0, 1, 0, 0]]             # x2 = -1, 1, 3, out of range
    assert R.check_true(np.zeros((1, 2), np.int32), np.array([[R.INT32_MIN, 5]], np.int32), -1, 256).tolist() == [[0, 1]]   # the marker


# ---- refusals before a device is touched ----
@pytest.fixture(scope="module")
def lib():
    return view2.bind(_bind_sgm(_lib.load()))


def status_of(rc):
    return rc, _lib.load().fsgm_last_error().decode()


def sgm_call(lib, *, n=1, W=8, H=4, D=16, P1=7, P2=100, prm=None, v2=None, exact=0, Cnull=False, bestD=True, minC=True, minC2=False,
             disp2=True, guide=None, dptr=False):
    Cv = np.zeros((n, H, W, D), np.uint8)
    u = lambda: np.zeros((n, H, W), np.uint32)
    a, b, c, d = u(), u(), u(), u()
    prm = prm if prm is not None else sgm_params(lib)
    v2 = v2 if v2 is not None else view2.params(lib)
    args = [n, None if Cnull else _lib.ptr(Cv), W, H, D, P1, P2, C.byref(prm), C.byref(v2), guide, _lib.ptr(a) if bestD else None,
            _lib.ptr(b) if minC else None, _lib.ptr(c) if minC2 else None, None, exact, _lib.ptr(d) if disp2 else None, None, None]
    return lib.fsgm_sgm_view2_dptr(*args, None, None) if dptr else lib.fsgm_sgm_view2_batch_host(*args)


@pytest.mark.parametrize("dptr", [False, True])
def test_sgm_view2_refusals(lib, dptr):
    def bad_v2(**kw):
        v = view2.params(lib)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    res = view2.params(lib)
    res.reserved[3] = 1
    invalid = [dict(Cnull=True), dict(bestD=False), dict(minC=False), dict(disp2=False), dict(n=0), dict(W=0), dict(D=0), dict(D=1025),
               dict(exact=2), dict(v2=bad_v2(direction=0)), dict(v2=bad_v2(direction=2)), dict(v2=bad_v2(max_diff=-1)),
               dict(v2=bad_v2(d_min=1025)), dict(v2=bad_v2(d_min=-1025)), dict(v2=res), dict(exact=1, P2=256),
               dict(prm=sgm_params(lib, paths=5)), dict(prm=sgm_params(lib, adaptive_p2=1))]
    for kw in invalid:
        assert sgm_call(lib, dptr=dptr, **kw) == INVALID, kw
    for mode in range(2, 7):
        assert sgm_call(lib, dptr=dptr, prm=sgm_params(lib, agg_mode=mode)) == UNSUPPORTED
    assert sgm_call(lib, dptr=dptr, exact=1, minC2=True) == UNSUPPORTED
    assert sgm_call(lib, dptr=dptr, n=65536, W=1, H=1, D=1) == UNSUPPORTED
    assert sgm_call(lib, dptr=dptr) == 2                                     # a good call reaches the device (none here)


@pytest.mark.parametrize("dptr", [False, True])
def test_stereo_view2_refusals(lib, dptr):
    def call(*, n=1, W=8, H=4, D=16, d_min=0, max_diff=256, fb=0, direction=-1, I1=True, disp=True, disp2=True):
        img, out = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.int32)
        prm = lib.fsgm_stereo_params_default()
        prm.fb_check, prm.direction = fb, direction
        args = [n, _lib.ptr(img) if I1 else None, _lib.ptr(img), W, H, D, 6, 64, C.byref(prm), None, d_min, max_diff,
                _lib.ptr(out) if disp else None, _lib.ptr(out), None, _lib.ptr(out) if disp2 else None, None, None]
        return lib.fsgm_stereo_sgm_view2_dptr(*args, None, None) if dptr else lib.fsgm_stereo_sgm_view2_host(*args)
    for kw in (dict(I1=False), dict(disp=False), dict(disp2=False), dict(n=0), dict(W=0), dict(D=0), dict(max_diff=-1), dict(fb=1),
               dict(direction=0), dict(d_min=1025), dict(d_min=-1025)):
        assert call(**kw) == INVALID, kw
    assert call(D=600) == 2                                                  # no dMax <= 511 limit: the call reaches the device


def test_check_refusals(lib):
    a = np.zeros((1, 4, 8), np.int32)
    cf = np.zeros((1, 4, 8), np.uint8)
    def call(*, n=1, W=8, H=4, direction=-1, max_diff=256, disp=True, disp2=True, conf=True, device=0, dptr=False):
        args = [n, _lib.ptr(a) if disp else None, _lib.ptr(a) if disp2 else None, W, H, direction, max_diff, _lib.ptr(cf) if conf else None, device]
        return lib.fsgm_view2_check_dptr(*args, None, None) if dptr else lib.fsgm_view2_check_host(*args)
    for dptr in (False, True):
        for kw in (dict(disp=False), dict(disp2=False), dict(conf=False), dict(n=0), dict(W=0), dict(H=0), dict(direction=0), dict(max_diff=-1),
                   dict(device=-1), dict(device=64)):
            assert call(dptr=dptr, **kw) == INVALID, kw
        assert call(dptr=dptr) == 2
    with pytest.raises(TypeError):
        fsgm_amd.view2_check(np.zeros((4, 8), np.uint32), np.zeros((4, 8), np.int32))


def test_defaults_and_plan_nulls(lib):
    p = lib.fsgm_view2_params_default()
    assert (p.direction, p.d_min, p.max_diff, list(p.reserved)) == (-1, 0, 256, [0] * 5)
    assert lib.fsgm_epi_plan_set_view2(None, 1, -1) == INVALID
    assert lib.fsgm_epi_plan_download_view2(None, 0, None, None) == INVALID
    with pytest.raises(ValueError):
        fsgm_amd.stereo_sgm(np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8), 4, fb_check=1, second_view=True)


def test_launch_lds_at_every_dmax(lib):
    for D in range(1, 1025):
        b, T = view2.launch_lds(D), view2.tile(D)
        assert b <= 65536
        assert (T == 0 and b == 0) if D > 256 else (T in (64, 128, 256) and b == T * D * 2 + 1024)
    b = C.c_uint64()
    assert lib.fsgm_view2_launch_lds(0, C.byref(b)) == INVALID and lib.fsgm_view2_launch_lds(1025, C.byref(b)) == INVALID
    assert lib.fsgm_view2_launch_lds(16, None) == INVALID and view2.tile(0) == 0 and view2.tile(1025) == 0


# ---- the existing wrappers with the switch off call only the old symbols ----
class StubLib:
    """Entry points that record their name and argument count and return 0: an older build, with none of the view-2 symbols."""
    fsgm_sgm_params_default = staticmethod(SgmParams)
    fsgm_stereo_params_default = staticmethod(_lib.StereoParams)

    def __init__(self, entries):
        self.calls = []
        for name in entries:
            setattr(self, name, lambda *a, _name=name: self.calls.append((_name, len(a))) or 0)


OLD = ("fsgm_sgm_batch_host", "fsgm_sgm_device", "fsgm_sgm_last_kernel", "fsgm_sgm_ingest_lds", "fsgm_epi_plan_ingest_cost_device",
       "fsgm_stereo_sgm_host")


def test_switch_off_reaches_the_old_entries_alone(monkeypatch):
    stub = StubLib(OLD)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    assert not any("view2" in n for n in dir(stub))
    out = fsgm_amd.sgm_batch(np.zeros((1, 4, 8, 16), np.uint8))
    assert stub.calls == [("fsgm_sgm_batch_host", 12)] and len(out) == 2
    stub.calls.clear()
    out = fsgm_amd.sgm_batch(np.zeros((1, 4, 8, 16), np.uint8), second_view=False, direction=1, d_min=3, max_diff=0)
    assert stub.calls == [("fsgm_sgm_batch_host", 12)] and len(out) == 2
    stub.calls.clear()
    img = np.zeros((4, 8), np.uint8)
    out = fsgm_amd.stereo_sgm(img, img, 4, second_view=False, max_diff=7)
    assert stub.calls == [("fsgm_stereo_sgm_host", 13)] and len(out) == 2 and out[0].dtype == np.uint32


def test_switch_on_reaches_the_view2_entries(monkeypatch):
    names = ("fsgm_sgm_view2_batch_host", "fsgm_sgm_view2_dptr", "fsgm_stereo_sgm_view2_host", "fsgm_stereo_sgm_view2_dptr",
             "fsgm_view2_check_host", "fsgm_view2_check_dptr", "fsgm_view2_launch_lds", "fsgm_view2_tile", "fsgm_epi_plan_set_view2",
             "fsgm_epi_plan_download_view2")
    stub = StubLib(OLD + names)
    stub.fsgm_view2_params_default = view2.View2Params
    monkeypatch.setattr(_lib, "load", lambda: stub)
    out = fsgm_amd.sgm_batch(np.zeros((1, 4, 8, 16), np.uint8), second_view=True, runner_up=True, return_sum=True)
    assert stub.calls == [("fsgm_sgm_view2_batch_host", 18)]
    assert [o.shape for o in out] == [(1, 4, 8)] * 3 + [(1, 4, 8, 16)] + [(1, 4, 8)] * 3 and out[-1].dtype == np.uint8
    stub.calls.clear()
    img = np.zeros((2, 4, 8), np.uint8)
    out = fsgm_amd.stereo_sgm(img, img, 4, second_view=True)
    assert stub.calls == [("fsgm_stereo_sgm_view2_host", 18)]
    assert [o.dtype for o in out] == [np.int32, np.uint32, np.int32, np.uint32, np.uint8]
    stub.calls.clear()
    assert fsgm_amd.view2_check(np.zeros((4, 8), np.int32), np.zeros((4, 8), np.int32)).shape == (4, 8)
    assert stub.calls == [("fsgm_view2_check_host", 9)]


# ---- the torch ops: a namespace of their own, schemas and fake outputs ----
def test_torch_ops_schemas_and_fakes():
    pytest.importorskip("torch")
    from fsgm_amd import torch_ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    ns = torch.ops.fsgm_view2
    assert str(ns.sgm.default._schema) == (
        "fsgm_view2::sgm(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, "
        "SymInt adaptive_p2, SymInt subpixel, SymInt return_sum, bool runner_up, bool exact, SymInt direction, SymInt d_min, SymInt max_diff) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(ns.stereo_sgm.default._schema) == (
        "fsgm_view2::stereo_sgm(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, "
        "SymInt direction, SymInt adaptive_p2, bool runner_up, SymInt max_diff) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(ns.check.default._schema) == "fsgm_view2::check(Tensor disp, Tensor disp2, SymInt direction, SymInt max_diff) -> (Tensor, Tensor)"
    for name in ("sgm_view2", "stereo_sgm_view2", "view2_check"):                # the fsgm:: namespace stays closed
        assert not hasattr(torch.ops.fsgm, name)
    u32, i32, u8 = torch.uint32, torch.int32, torch.uint8
    sig = lambda r: [(tuple(t.shape), t.dtype) for t in r]
    with FakeTensorMode():
        Cv = torch.empty((3, 16, 9, 33), dtype=u8, device="cuda")
        r = ops.sgm(Cv, second_view=True, runner_up=True, return_sum=True, return_status=True)
        assert sig(r) == [((3, 9, 33), u32)] * 3 + [((3, 9, 33, 16), u32)] + [((3, 9, 33), u32)] * 2 + [((3, 9, 33), u8), ((), i32)]
        r = ops.sgm(Cv[0].permute(1, 2, 0).contiguous(), layout="hwd", arith="exact", second_view=True, direction=1, d_min=5, max_diff=0)
        assert sig(r) == [((9, 33), u32)] * 4 + [((9, 33), u8)]
        assert sig(ops.sgm(Cv)) == [((3, 9, 33), u32)] * 2                         # the switch off: what it was
        empty = torch.empty((0,), dtype=u8, device="cuda")
        out = ns.sgm(Cv, empty, 7, 100, 4, 1, 255, 0, 0, 1, 0, False, False, -1, 0, 256)
        assert [tuple(t.shape) for t in out] == [(3, 9, 33)] * 2 + [(0,), (0,)] + [(3, 9, 33)] * 3 + [()]
        img = torch.empty((2, 9, 33), dtype=u8, device="cuda")
        r = ops.stereo_sgm(img, img, 8, second_view=True, runner_up=True, return_status=True)
        assert sig(r) == [((2, 9, 33), i32), ((2, 9, 33), u32), ((2, 9, 33), u32), ((2, 9, 33), i32), ((2, 9, 33), u32), ((2, 9, 33), u8), ((), i32)]
        r = ops.stereo_sgm(img[0], img[0], 8, second_view=True, d_min=-3)
        assert sig(r) == [((9, 33), i32), ((9, 33), u32), ((9, 33), i32), ((9, 33), u32), ((9, 33), u8)]
        assert sig(ops.stereo_sgm(img, img, 8)) == [((2, 9, 33), u32)] * 2
        assert [tuple(t.shape) for t in ns.stereo_sgm(img, img, 8, 0, 6, 64, 4, 1, -1, 0, False, 256)][2] == (0,)
        d = torch.empty((2, 9, 33), dtype=i32, device="cuda")
        assert sig([ops.view2_check(d, d)]) == [((2, 9, 33), u8)] and sig([ops.view2_check(d[0], d[0], direction=1)]) == [((9, 33), u8)]
        with pytest.raises(ValueError):
            ops.stereo_sgm(img, img, 8, second_view=True, fb_check=1)
        with pytest.raises(TypeError):
            ops.view2_check(d.to(torch.int64), d)
        with pytest.raises(ValueError):
            ops.view2_check(d, d, direction=0)
