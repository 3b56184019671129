"""CPU tests of the runner-up cost and the uniqueness filter: the numpy restatement on hand-written rows, the refusals that answer
before a device is touched, the ratio's meaning, and the torch ops' schemas and fake implementations."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib  # noqa: E402
from tests import runner_up_restatement as RU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4
NONE = RU.NO_RUNNER_UP
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first


def _ru(row):
    b, c, c2 = RU.runner_up(np.array(row, np.uint32))
    return int(b), int(c), int(c2)


# ---- the restatement on hand-written rows ----
def test_no_runner_up_at_one_two_and_three_candidates():
    assert _ru([7]) == (0, 7, NONE)
    assert _ru([3, 9]) == (0, 3, NONE) and _ru([9, 3]) == (1, 3, NONE)
    assert _ru([1, 5, 9]) == (0, 1, 9)                          # best 0: d = 2 is two away
    assert _ru([5, 1, 9]) == (1, 1, NONE)                       # best 1: both others adjacent
    assert _ru([9, 5, 1]) == (2, 1, 9)                          # best 2: d = 0


def test_constant_rows():
    assert _ru([4]) == (0, 4, NONE) and _ru([4, 4]) == (0, 4, NONE)
    for D in (3, 4, 16, 300):
        assert _ru([4] * D) == (0, 4, 4)                         # the first minimum wins, minC2 == minC


def test_best_at_either_end():
    assert _ru([0, 9, 8, 7, 6]) == (0, 0, 6)
    assert _ru([6, 7, 8, 9, 0]) == (4, 0, 6)
    assert _ru([9, 9, 9, 2, 0]) == (4, 0, 9)                    # the 2 next to the end is skipped


def test_adjacent_second_smallest_is_skipped():
    assert _ru([7, 9, 1, 0, 8, 9]) == (3, 0, 7)                  # 1 at best - 1, 8 at best + 1: both inside the window
    assert _ru([7, 9, 8, 0, 1, 9]) == (3, 0, 7)                  # 1 at best + 1
    assert _ru([9, 5, 1, 0, 1, 6]) == (3, 0, 5)


def test_tie_two_apart_and_one_apart():
    assert _ru([9, 3, 8, 3, 9]) == (1, 3, 3)                     # the later minimum is two away: minC2 == minC
    assert _ru([9, 3, 3, 8, 9]) == (1, 3, 8)                     # one away: inside the window
    S = np.array([[[5, 1, 5, 1], [2, 2, 2, 2]]], np.uint32)      # shapes with leading axes
    b, c, c2 = RU.runner_up(S)
    assert b.tolist() == [[1, 0]] and c.tolist() == [[1, 2]] and c2.tolist() == [[1, 2]]
    assert c.dtype == np.uint32 and c2.dtype == np.uint32


# ---- the ratio ----
def test_ratio_semantics():
    rng = np.random.default_rng(5)
    minC = rng.integers(0, 2041, 500).astype(np.uint32)
    minC2 = np.maximum(minC, rng.integers(0, 2041, 500)).astype(np.uint32)
    minC2[::7] = NONE
    minC[::11] = 0
    assert not RU.uniqueness_reject(minC, minC2, 0).any()        # minC2 >= minC: ratio 0 rejects nothing
    all_ = RU.uniqueness_reject(minC, minC2, 100)
    assert np.array_equal(all_, (minC2 != NONE) & (minC > 0))    # ratio 100: every pixel with a runner-up and minC > 0
    r15 = RU.uniqueness_reject(minC, minC2, 15)
    assert r15.any() and not r15.all() and not (r15 & ~all_).any()
    # exact at the boundary: 85 * 100 == 85 * 100 keeps, one less rejects
    assert RU.uniqueness_reject(np.uint32([85]), np.uint32([100]), 15).tolist() == [False]
    assert RU.uniqueness_reject(np.uint32([86]), np.uint32([100]), 15).tolist() == [True]
    # products beyond 32 bits
    big = np.uint32([2 ** 32 // 100 + 5])
    assert RU.uniqueness_reject(big, big, 0).tolist() == [False] and RU.uniqueness_reject(big, big, 1).tolist() == [True]
    m = np.array([1.5, np.nan, 2.0])
    out = RU.uniqueness_filter(m, np.uint32([10, 10, 10]), np.uint32([10, 99, NONE]), 15)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 2.0 and m[0] == 1.5


# ---- refusals before a device ----
def _err(lib):
    return lib.fsgm_last_error().decode()


def test_header_and_python_agree_on_the_marker():
    hdr = open(os.path.join(ROOT, "include", "fsgm.h")).read()
    assert "#define FSGM_NO_RUNNER_UP 0xFFFFFFFFu" in hdr
    assert fsgm_amd.NO_RUNNER_UP == NONE == 0xFFFFFFFF


def test_stereo_ru_entry_points_refuse_before_any_device():
    lib = _lib.load()
    host = lambda n=1, W=8, H=4, D=16, d_min=0, m2=FAKE: lib.fsgm_stereo_sgm_host_ru(                      # noqa: E731
        n, FAKE, FAKE, W, H, D, 6, 64, None, None, d_min, FAKE, FAKE, m2, None, None)
    dev = lambda n=1, W=8, H=4, D=16, d_min=0, m2=FAKE: lib.fsgm_stereo_sgm_device_ru(                     # noqa: E731
        n, FAKE, FAKE, W, H, D, 6, 64, None, None, d_min, FAKE, FAKE, m2, None, None, None, None)
    for fn in (host, dev):
        assert fn(m2=None) == INVALID and "minC2" in _err(lib)
        assert fn(n=0) == INVALID and "n_frames" in _err(lib)
        assert fn(W=0) == INVALID and "width/height" in _err(lib)
        assert fn(H=-1) == INVALID and fn(D=0) == INVALID
        assert fn(d_min=1025) == INVALID and "d_min" in _err(lib)


def test_uniqueness_filter_refuses_before_any_device():
    lib = _lib.load()
    m = np.zeros((2, 4, 6))
    c, c2 = np.zeros((2, 4, 6), np.uint32), np.zeros((2, 4, 6), np.uint32)
    p = _lib.ptr
    host = lambda n=2, W=6, H=4, ratio=15, a=p(m), b=p(c), d=p(c2), o=p(m), device=0: lib.fsgm_uniqueness_filter_host(   # noqa: E731
        n, a, b, d, W, H, ratio, o, device)
    dev = lambda n=2, W=6, H=4, ratio=15, a=p(m), b=p(c), d=p(c2), o=p(m), device=0: lib.fsgm_uniqueness_filter_device(  # noqa: E731
        n, a, b, d, W, H, ratio, o, device, None, None)
    for fn in (host, dev):
        for ratio in (-1, 101):
            assert fn(ratio=ratio) == INVALID and "ratio" in _err(lib)
        for k in ("a", "b", "d", "o"):
            assert fn(**{k: None}) == INVALID and "null" in _err(lib)
        assert fn(n=0) == INVALID and "n_frames" in _err(lib)
        assert fn(W=0) == INVALID and fn(H=0) == INVALID and "width/height" in _err(lib)
        assert fn(o=p(c)) == INVALID and "overlap" in _err(lib)                      # out over minC
        assert fn(o=p(c2)) == INVALID and "overlap" in _err(lib)
        assert fn(o=C.c_void_p(m.ctypes.data + 8)) == INVALID and "map itself" in _err(lib)
        assert fn(device=64) == INVALID and "out of range" in _err(lib)
    assert not m.any()


def test_plan_switch_argument_checks():
    lib = _lib.load()
    assert lib.fsgm_epi_plan_set_runner_up(None, 1) == INVALID and "null plan" in _err(lib)
    assert lib.fsgm_epi_plan_download_runner_up(None, 0, FAKE) == INVALID and "null" in _err(lib)
    assert isinstance(lib.fsgm_stereo_sgm_last_kernel(), bytes)


def test_python_wrappers_validate_before_the_library():
    m = np.zeros((4, 6))
    c = np.zeros((4, 6), np.uint32)
    for ratio in (-1, 101, 2.5, True):
        with pytest.raises(ValueError, match="ratio"):
            fsgm_amd.uniqueness_filter(m, c, c, ratio)
    with pytest.raises(TypeError, match="float64"):
        fsgm_amd.uniqueness_filter(m.astype(np.float32), c, c, 5)
    with pytest.raises(TypeError, match="minC2"):
        fsgm_amd.uniqueness_filter(m, c, c[:2], 5)
    with pytest.raises(TypeError, match="minC"):
        fsgm_amd.uniqueness_filter(m, c.astype(np.int32), c, 5)
    assert inspect.signature(fsgm_amd.stereo_sgm).parameters["runner_up"].default is False
    assert inspect.signature(torch_ops.stereo_sgm).parameters["runner_up"].default is False


# ---- the torch ops ----
def test_schemas():
    assert str(torch.ops.fsgm.stereo_sgm_ru.default._schema) == (
        "fsgm::stereo_sgm_ru(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, "
        "SymInt direction, SymInt fb_check, SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.uniqueness_filter.default._schema) == (
        "fsgm::uniqueness_filter(Tensor map_, Tensor minC, Tensor minC2, SymInt ratio) -> (Tensor, Tensor)")
    # the neighbours are what they were
    assert str(torch.ops.fsgm.stereo_sgm.default._schema) == (
        "fsgm::stereo_sgm(Tensor left, Tensor right, SymInt dMax, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, "
        "SymInt fb_check, SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.fsgm.stereo_sgm_range.default._schema) == (
        "fsgm::stereo_sgm_range(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, "
        "SymInt direction, SymInt fb_check, SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")


def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    meta = lambda ts: [(tuple(t.shape), t.dtype, t.device.type) for t in ts]          # noqa: E731
    with FakeTensorMode():
        for lead in ((), (3,)):
            shp = lead + (8, 12)
            L = torch.empty(shp, dtype=torch.uint8, device="cuda")
            r = torch_ops.stereo_sgm(L, L, 16, runner_up=True, return_status=True)
            assert meta(r) == [(shp, torch.uint32, "cuda")] * 3 + [((), torch.int32, "cuda")]
            r = torch_ops.stereo_sgm(L, L, 16, runner_up=True, d_min=-3, fb_check=1)
            assert meta(r) == [(shp, t, "cuda") for t in (torch.int32, torch.uint32, torch.uint8, torch.int32, torch.uint32)]
            r = torch_ops.stereo_sgm(L, L, 16, runner_up=True, fb_check=1)
            assert meta(r) == [(shp, t, "cuda") for t in (torch.uint32, torch.uint32, torch.uint8, torch.uint32, torch.uint32)]
            r = torch_ops.stereo_sgm(L, L, 16)                                         # the default: the pair it always returned
            assert meta(r) == [(shp, torch.uint32, "cuda")] * 2
            m = torch.empty(shp, dtype=torch.float64, device="cuda")
            c = torch.empty(shp, dtype=torch.uint32, device="cuda")
            assert meta([torch_ops.uniqueness_filter(m, c, c, 15)]) == [(shp, torch.float64, "cuda")]
            with pytest.raises(ValueError, match="ratio"):
                torch_ops.uniqueness_filter(m, c, c, 101)
            with pytest.raises(TypeError, match="uint32"):
                torch_ops.uniqueness_filter(m, c.to(torch.int32), c, 5)
            with pytest.raises(TypeError, match="shape"):
                torch_ops.uniqueness_filter(m, c, c[..., :4], 5)
        raw = torch.ops.fsgm.stereo_sgm_ru(torch.empty((2, 8, 12), dtype=torch.uint8, device="cuda"),
                                           torch.empty((2, 8, 12), dtype=torch.uint8, device="cuda"), 16, 0, 6, 64, 4, 1, -1, 0)
        assert meta(raw) == [((2, 8, 12), torch.int32, "cuda")] + [((2, 8, 12), torch.uint32, "cuda")] * 2 + [
            ((0,), torch.uint8, "cuda"), ((0,), torch.int32, "cuda"), ((), torch.int32, "cuda")]
        raw = torch.ops.fsgm.uniqueness_filter(torch.empty((2, 8, 12), dtype=torch.float64, device="cuda"),
                                               torch.empty((2, 8, 12), dtype=torch.uint32, device="cuda"),
                                               torch.empty((2, 8, 12), dtype=torch.uint32, device="cuda"), 15)
        assert meta(raw) == [((2, 8, 12), torch.float64, "cuda"), ((), torch.int32, "cuda")]
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.uniqueness_filter(torch.zeros(4, 6, dtype=torch.float64), torch.zeros(4, 6, dtype=torch.uint32),
                                    torch.zeros(4, 6, dtype=torch.uint32), 5)


# ---- the crafted volumes meet every edge: checked here on the oracle's S before the GPU test relies on it ----
@pytest.mark.parametrize("D", __import__("tests.runner_up_volumes", fromlist=["ALL_D"]).ALL_D)
def test_crafted_volumes_meet_every_edge(oracle, D):
    from tests import runner_up_volumes as V
    for paths, batch in ((4, 1), (8, 3)):
        total = {}
        for Cv in V.volumes(D, batch, seed=100 * D + paths):
            assert Cv.shape == (V.H, V.W, D) and Cv.dtype == np.uint8 and Cv.max() <= 24
            S = np.asarray(oracle.epi_aggregate(Cv, V.P1, V.P2, paths))[:V.H * V.W * D].reshape(V.H, V.W, D)
            best, minC, minC2 = RU.runner_up(S)
            for k, v in V.edge_counts(D, best, minC, minC2, S).items():
                total[k] = total.get(k, 0) + v
        for k in V.required(D, batch):
            assert total[k] > 0, f"D {D}, {paths} paths, batch {batch}: no pixel with {k} ({total})"
