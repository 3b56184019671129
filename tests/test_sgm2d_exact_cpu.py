"""CPU-side tests of the 2-D matcher with exact path arithmetic (fsgm_sgm2d_batch_host_exact / fsgm_sgm2d_device_exact,
fsgm_pyd_plan_set_exact, fsgm::sgm2d_exact): the yardstick of the GPU tests (tests/sgm2d_exact_restatement.py) tied to the pinned
oracle where the two must agree, the proof that they disagree where the GPU tests look, and every refusal of the new entries
that needs no device."""
import ctypes as C

import numpy as np
import pytest

try:                                     # torch first where it is installed: the library must bind to its HIP runtime
    import torch  # noqa: F401
except ImportError:                      # (only the torch test at the end needs it)
    torch = None

from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.sgm2d import _bind, sgm2d_batch  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import sgm2d_exact_cases as K  # noqa: E402
from tests import sgm2d_exact_restatement as X  # noqa: E402

FSGM_ERR_INVALID = 1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call it goes into fails its argument checks first


@pytest.fixture(scope="module")
def lib():
    return _bind(_lib.load())


def _err(lib):
    return lib.fsgm_last_error().decode()


# ---- 1. inside the no-wrap budget the restatement IS the pinned oracle ----
@pytest.mark.parametrize("hints", ["zero", "general", "beyond"])
@pytest.mark.parametrize("adaptive", [0, 1], ids=["plain", "adaptive"])
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("rX,rY", [(0, 0), (1, 1), (4, 4), (2, 5), (6, 6)], ids=["1x1", "3x3", "9x9", "5x11", "13x13"])
def test_restatement_equals_the_oracle_inside_the_budget(rX, rY, diagonal, passes, adaptive, hints):
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    for (cmax, P1, P2), (W, H) in zip(((24, 6, 64), (55, 7, 100), (255, 0, 0)), ((11, 7), (7, 5), (9, 1))):
        assert cmax + P2 + max(P1, P2) <= 255
        seed = 1000 * cmax + 10 * Sx + Sy + 2 * diagonal + passes + 4 * adaptive
        Cv = np.random.default_rng(seed).integers(0, cmax + 1, (H, W, Sx * Sy), dtype=np.uint8)
        Cv[-1, -1, -1] = cmax                                   # the bound is reached
        mv = np.zeros((2, H, W)) if hints == "zero" else K.hints(hints, W, H, rX, rY, 1, seed)[0]
        I1 = K.guides(W, H, 1, seed)[0] if adaptive else np.zeros((H, W), np.uint8)
        S = X.aggregate(Cv, mv, Sx, Sy, P1, P2, diagonal, passes, I1 if adaptive else None)
        oS = pyoracle.pyd_aggregate(I1, Cv, mv, Sx, Sy, P1, P2, diagonal, passes, adaptive)
        assert np.array_equal(S, oS), f"cmax {cmax} P {P1}/{P2} {W}x{H}"


def _second_pixels_reach_510(paths, H, W):
    """on each path of each pass, every pixel that follows a path's first pixel (and starts no path itself) holds L = 510 at every
    candidate"""
    for p, name, L, started in paths:
        dy, dx = {"L1": (0, 1), "L3": (1, 0), "L2": (1, 1), "L4": (1, -1)}[name]
        sgn = 1 if p == 0 else -1                                # (later passes run the mirrored frame: xstep = ystep = -1)
        n = 0
        for y0, x0 in zip(*np.nonzero(started)):
            y1, x1 = y0 + sgn * dy, x0 + sgn * dx
            if 0 <= y1 < H and 0 <= x1 < W and not started[y1, x1]:
                assert (L[y1, x1] == 510).all(), (p, name, y1, x1)
                n += 1
        assert n > 0


# ---- 2. outside it the two differ, at every input the GPU tests use ----
@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_gpu_cases_lie_where_mod256_and_exact_differ(c):
    """Were the exact entries to run the old kernels, the GPU comparisons with the restatement could not pass: some path cost
    exceeds a byte and the summed costs differ from the oracle's mod-256 ones.  One kind of case cannot show that and says so:
    P1 = P2 = 0 lies inside the budget (255 + 0 + 0), where exact and mod 256 are the same numbers.  (A 1x1 window is no
    exception: behind a path start the stored minimum is 0, so L = C + min(Lp, P2) exceeds a byte there.)"""
    Sx, Sy = 2 * c.rX + 1, 2 * c.rY + 1
    vols, hints, guides = K.inputs(c)
    ndirs = (4 if c.diagonal else 2) * c.passes
    lmax, differs = 0, False
    for f in range(c.n):
        mv = np.zeros((2, c.H, c.W)) if hints is None else hints[f]
        I1 = guides[f] if c.adaptive else np.zeros((c.H, c.W), np.uint8)
        paths = []
        S = X.aggregate(vols[f], mv, Sx, Sy, c.P1, c.P2, c.diagonal, c.passes, guides[f] if c.adaptive else None, paths_out=paths)
        assert len(paths) == ndirs
        assert np.array_equal(S.astype(np.uint32), K.want(c)[4][f])
        assert S.max() <= ndirs * (255 + c.P2)
        for _, _, L, _ in paths:
            y = L - vols[f].astype(np.int64)
            assert y.min() >= 0 and y.max() <= c.P2 and L.max() <= 255 + c.P2          # what the kernels store is one byte
            lmax = max(lmax, int(L.max()))
        oS = pyoracle.pyd_aggregate(I1, vols[f], mv, Sx, Sy, c.P1, c.P2, c.diagonal, c.passes, c.adaptive)
        differs |= not np.array_equal(S, oS)
        if c.volume == "all255" and c.P2 == 255:
            _second_pixels_reach_510(paths, c.H, c.W)
            assert lmax == 510
    print(f"{K.case_id(c)}: max L {lmax}, S differs from mod 256: {differs}")
    if not K.outside_budget(c):
        assert (c.P1, c.P2) == (0, 0) and lmax <= 255 and not differs
    else:
        assert lmax > 255, "no path cost leaves a byte"
        assert differs, "the exact sums equal the mod-256 ones"


def test_all_255_reaches_510_at_each_paths_second_pixel():
    """the all-255 volume at P2 = 255, zero hints: a path's first pixel stores L = 255 and minimum 0, so its second pixel has
    L = 255 + min(255, 255 + P1, 0 + 255) - 0 = 510 at every candidate, on every path of both passes"""
    H, W, Sx, Sy = 5, 7, 3, 3
    Cv = np.full((H, W, 9), 255, np.uint8)
    paths = []
    S = X.aggregate(Cv, np.zeros((2, H, W)), Sx, Sy, 255, 255, 1, 2, paths_out=paths)
    assert len(paths) == 8
    _second_pixels_reach_510(paths, H, W)
    assert S.max() <= 8 * 510


# ---- 3. refusals without a device ----
def _host(lib, P1=7, P2=100, Cp=FAKE, bestD=FAKE, minC=FAKE, mvSub=FAKE, prm=None):
    return lib.fsgm_sgm2d_batch_host_exact(1, Cp, 8, 6, 1, 1, P1, P2, None if prm is None else C.byref(prm), None, 0, 0, None, bestD, minC,
                                           None, mvSub, None, None)


def _device(lib, P1=7, P2=100, Cp=FAKE, bestD=FAKE, minC=FAKE, mvSub=FAKE, prm=None):
    return lib.fsgm_sgm2d_device_exact(1, Cp, 8, 6, 1, 1, P1, P2, None if prm is None else C.byref(prm), None, 0, 0, None, bestD, minC,
                                       None, mvSub, None, None, None, None)


@pytest.mark.parametrize("call", [_host, _device], ids=["host", "device"])
def test_exact_entries_refuse_without_a_device(lib, call):
    for P1 in (-1, 256):
        assert call(lib, P1=P1) == FSGM_ERR_INVALID and "P1 in 0..255" in _err(lib)
    for P2 in (-1, 256):
        assert call(lib, P2=P2) == FSGM_ERR_INVALID and "P2 in 0..255" in _err(lib)
    for null in ("Cp", "bestD", "minC", "mvSub"):
        assert call(lib, **{null: None}) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    p = lib.fsgm_sgm2d_params_default()
    p.reserved[0] = 1                                            # (no reserved word was spent on the switch)
    assert call(lib, prm=p) == FSGM_ERR_INVALID and "reserved" in _err(lib)
    p = lib.fsgm_sgm2d_params_default()
    p.cost_bound = 0
    assert call(lib, prm=p) == FSGM_ERR_INVALID and "cost_bound" in _err(lib)


def test_plan_switch_refuses_a_null_plan(lib):
    from fsgm_amd import pyd
    pyd._bind(lib)
    assert lib.fsgm_pyd_plan_set_exact(None, 1) == FSGM_ERR_INVALID and "null plan" in _err(lib)


def test_python_wrappers():
    Cv = np.zeros((9, 5, 7), np.uint8)
    with pytest.raises(ValueError, match="arith"):
        sgm2d_batch(Cv, 1, 1, arith="saturate")
    with pytest.raises(ValueError, match="arith"):
        sgm2d_batch(Cv, 1, 1, arith="mod256")                    # (the 1-D door's name for the default is not this door's)
    for P1, P2 in ((7, 256), (-1, 100)):
        with pytest.raises(_lib.FsgmError) as e:
            sgm2d_batch(Cv, 1, 1, P1, P2, arith="exact")
        assert e.value.status == FSGM_ERR_INVALID
        with pytest.raises(_lib.FsgmError) as e:
            sgm2d_batch(Cv, 1, 1, P1, P2, arith="exact", runner_up=True)
        assert e.value.status == FSGM_ERR_INVALID


def test_torch_op_is_registered_and_has_a_fake():
    pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from fsgm_amd import torch_ops
    assert hasattr(torch.ops.fsgm, "sgm2d_exact")
    ru, ex = (str(getattr(torch.ops.fsgm, n).default._schema).split("(", 1)[1] for n in ("sgm2d_ru", "sgm2d_exact"))
    assert ex == ru.replace(") -> ", ", bool runner_up) -> ")   # fsgm::sgm2d_ru's schema with the one argument added
    with FakeTensorMode():
        Cv = torch.empty((3, 81, 9, 33), dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm2d(Cv, 4, 4, 7, 100, arith="exact", return_flow=True, return_sum=True, return_status=True)
        u32, f64 = torch.uint32, torch.float64
        assert [(tuple(t.shape), t.dtype) for t in r] == [((3, 9, 33), u32)] * 2 + [((3, 2, 9, 33), f64)] * 2 + [((3, 9, 33, 81), u32),
                                                                                                               ((), torch.int32)]
        r = torch_ops.sgm2d(Cv, 4, 4, 7, 100, arith="exact", runner_up=True)
        assert [(tuple(t.shape), t.dtype) for t in r] == [((3, 9, 33), u32)] * 3 + [((3, 2, 9, 33), f64)]
        bd, mc, m2, ms, fl, S, st = torch.ops.fsgm.sgm2d_exact(Cv, torch.empty((0,), dtype=f64, device="cuda"),
                                                               torch.empty((0,), dtype=torch.uint8, device="cuda"), 4, 4, 7, 100, 1, 255,
                                                               1, 2, 0, 1, 0, 0, False)
        assert m2.numel() == 0 and fl.numel() == 0 and S.numel() == 0
        with pytest.raises(ValueError, match="arith"):
            torch_ops.sgm2d(Cv, 4, 4, arith="exact256")
