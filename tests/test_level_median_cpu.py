"""CPU tests of the median between pyramid levels: the numpy restatement (tests/level_median_restatement.py) against the rule
already in the tree (oracle.vmf) and against a brute-force sort, its level loops with the median off against the oracle's, every
refusal of the new entry points that answers before a device is touched, and the new torch ops' fake implementations."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, pyramid as _pyramid  # noqa: E402
from tests import edge_inputs as E  # noqa: E402
from tests import level_median_restatement as LM  # noqa: E402

INVALID = 1
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first
BAD_SIZES = (1, 4, -3)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)   # (numpy equality: -0.0 == 0.0)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("seed", range(6))
def test_medfilt2_5_is_the_oracles_vmf(oracle, seed):
    r = E.rng(700 + seed)
    W, H = [(1, 1), (3, 2), (7, 9), (64, 5), (33, 21), (65, 4)][seed]
    flows = E.vmf_flows(r, W, H, 2, 2)
    for f in flows:
        _same(np.stack([LM.medfilt2(c, 5) for c in f]), oracle.vmf(f), f"{W}x{H}")


def _brute_median(plane, s):
    """the definition, one window at a time: numbers in ascending order (Python's sort on floats without NaN), then the NaNs"""
    H, W = plane.shape
    r, out = s // 2, np.empty((H, W))
    for y in range(H):
        for x in range(W):
            vals = [plane[yy, xx] if 0 <= yy < H and 0 <= xx < W else 0.0
                    for yy in range(y - r, y + r + 1) for xx in range(x - r, x + r + 1)]
            numbers = sorted(v for v in vals if v == v)
            out[y, x] = (numbers + [np.nan] * (len(vals) - len(numbers)))[(s * s - 1) // 2]
    return out


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1), (2, 3), (9, 8)])
def test_medfilt2_3_against_a_brute_force_sort(W, H):
    for seed in range(4):
        flows = E.vmf_flows(E.rng(720 + seed), W, H, 2, 2)
        for plane in flows.reshape(-1, H, W):
            _same(LM.medfilt2(plane, 3), _brute_median(plane, 3), f"{W}x{H} seed {seed}")
    nans = np.full((H, W), np.nan)                               # NaN only where more than half the window is inside the map
    _same(LM.medfilt2(nans, 3), _brute_median(nans, 3))


def test_level_hints_shape_and_values():
    flow = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    np.testing.assert_array_equal(LM.level_hints(flow, 0), 2 * np.repeat(np.repeat(flow, 2, 1), 2, 2))
    h = LM.level_hints(flow, 3)
    assert h.shape == (2, 4, 6)
    # plane 0 = [[0 1 2] [3 4 5]]: the windows of the middle column hold all six values and three zeros of padding, sorted
    # 0 0 0 0 1 2 3 4 5, so the 5th smallest is 1; the corner (0, 0) sees 0 1 3 4 and five zeros
    assert h[0, 0, 2] == 2.0 and h[0, 3, 3] == 2.0 and h[0, 0, 0] == 0.0


@pytest.mark.parametrize("W,H,ch,numPyd", [(64, 48, 1, 3), (61, 47, 3, 3), (5, 4, 1, 2), (33, 21, 1, 1)])
def test_the_loops_without_the_median_are_the_oracles(oracle, W, H, ch, numPyd):
    I0, I1 = E.image_pair(E.rng(1), W, H, ch, seed=3)
    mv, minC, lv = oracle.pyramidal_sgm(I0, I1, numPyd)
    gmv, gminC, glv, _ = LM.pyramidal_sgm_lm(oracle, I0, I1, numPyd, 0)
    np.testing.assert_array_equal(gmv, mv)
    np.testing.assert_array_equal(gminC, minC)
    for a, b in zip(glv, lv):
        np.testing.assert_array_equal(a, b)
    flows, mc = E.oracle_pyramidal_ng(oracle, I0, I1, numPyd)
    gflows, gmc, _ = LM.pyramidal_ng_lm(oracle, I0, I1, numPyd, 0)
    np.testing.assert_array_equal(gmc, mc)
    for a, b in zip(gflows, flows):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------- refusals, no device touched
def _libs():
    lib = _lib.load()
    _pyramid._bind(lib)
    _pyramid._bind_ng(lib)
    _pyramid._bind_flow_pp(lib)
    return lib


def _refused(lib, st, word):
    assert st == INVALID, lib.fsgm_last_error().decode()
    assert word in lib.fsgm_last_error().decode()


@pytest.mark.parametrize("size", BAD_SIZES)
def test_a_bad_size_is_invalid_from_every_new_entry(size):
    lib = _libs()
    assert torch_ops._L is lib                                   # (torch_ops has declared the device forms' argument types)
    pyd, ng = lib.fsgm_pyramid_params_default(), lib.fsgm_ng_pyramid_params_default()
    for prm, host, dev in ((pyd, lib.fsgm_pyramidal_sgm_host_lm, lib.fsgm_pyramidal_sgm_device_lm),
                           (ng, lib.fsgm_pyramidal_sgm_ng_host_lm, lib.fsgm_pyramidal_sgm_ng_device_lm)):
        _refused(lib, host(FAKE, FAKE, 32, 24, 1, C.byref(prm), size, FAKE, FAKE, None, None), "level_median")
        _refused(lib, host(FAKE, FAKE, 32, 24, 1, C.byref(prm), size, FAKE, FAKE, FAKE, None), "level_median")
        _refused(lib, dev(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), size, FAKE, FAKE, None, None, None), "level_median")
    for matcher in ("pyd", "ng"):
        prm = _pyramid.flow_pp_params(lib, matcher, 2, 0, 0, {})
        for ratio, m2 in ((0, None), (15, FAKE)):
            _refused(lib, lib.fsgm_pyramidal_flow_pp_host_lm(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), ratio, size, FAKE, None, None, None,
                                                             None, m2), "level_median")
            _refused(lib, lib.fsgm_pyramidal_flow_pp_device_lm(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), ratio, size, FAKE, None, None, None,
                                                               None, m2, None, None), "level_median")
    _refused(lib, lib.fsgm_flow_level_hints_host(1, FAKE, 32, 24, size, FAKE, 0), "level_median")
    _refused(lib, lib.fsgm_flow_level_hints_device(1, FAKE, 32, 24, size, FAKE, 0, None), "level_median")
    # the plan switches answer for the size ahead of everything else (a plan needs a device, so none is made here)
    _refused(lib, lib.fsgm_pyramid_plan_set_level_median(None, size), "level_median")
    _refused(lib, lib.fsgm_ng_pyramid_plan_set_level_median(None, size), "level_median")


def test_a_null_minC2_with_a_ratio_is_refused():
    lib = _libs()
    for matcher in ("pyd", "ng"):
        prm = _pyramid.flow_pp_params(lib, matcher, 2, 0, 0, {})
        for lm in (0, 3, 5):
            _refused(lib, lib.fsgm_pyramidal_flow_pp_host_lm(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), 15, lm, FAKE, None, None, None, None,
                                                             None), "minC2")
            _refused(lib, lib.fsgm_pyramidal_flow_pp_device_lm(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), 15, lm, FAKE, None, None, None, None,
                                                               None, None, None), "minC2")
        for ratio in (-1, 101):
            _refused(lib, lib.fsgm_pyramidal_flow_pp_host_lm(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), ratio, 3, FAKE, None, None, None, None,
                                                             FAKE), "uniqueness_ratio")


def test_python_refuses_before_the_library_is_called(monkeypatch):
    I = np.zeros((8, 9), np.uint8)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    for size in BAD_SIZES + (True, 3.5, "3"):
        for fn in (fsgm_amd.pyramidal_sgm, fsgm_amd.pyramidal_sgm_ng, fsgm_amd.pyramidal_flow_pp):
            with pytest.raises(ValueError, match="level_median"):
                fn(I, I, 2, level_median=size)
        with pytest.raises(ValueError, match="level_median"):
            fsgm_amd.flow_level_hints(np.zeros((2, 3, 3)), size)
        with pytest.raises(ValueError, match="level_median"):
            _pyramid.level_median_of(size)
    for fn in (fsgm_amd.pyramidal_sgm_batch, fsgm_amd.pyramidal_sgm_ng_batch):
        with pytest.raises(ValueError, match="level_median"):
            fn([(I, I)], 2, devices=(0,), level_median=3)


# ---------------------------------------------------------------------------------------------- torch
def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    meta = lambda ts: [(tuple(t.shape), t.dtype, t.device.type) for t in ts]          # noqa: E731
    with FakeTensorMode():
        for lead in ((), (3,)):
            I = torch.empty(lead + (10, 21), dtype=torch.uint8, device="cuda")
            px, fl = lead + (10, 21), lead + (2, 10, 21)
            f64, u32, st = torch.float64, torch.uint32, ((), torch.int32, "cuda")
            for fn in (torch_ops.pyramidal_sgm, torch_ops.pyramidal_sgm_ng):
                r = fn(I, I, 2, batch=bool(lead), level_median=3, return_status=True)
                assert meta(r) == [(fl, f64, "cuda"), (px, u32, "cuda"), st]
                r = fn(I, I, 2, batch=bool(lead), level_median=5, runner_up=True, return_status=True)
                assert meta(r) == [(fl, f64, "cuda")] + [(px, u32, "cuda")] * 2 + [st]
            for matcher in ("pyd", "ng"):
                r = torch_ops.pyramidal_flow_pp(I, I, 2, matcher, batch=bool(lead), level_median=3)
                assert meta(r) == [(lead + (3, 10, 21), f64, "cuda")] + [(fl, f64, "cuda")] * 3 + [(px, u32, "cuda")]
                r = torch_ops.pyramidal_flow_pp(I, I, 2, matcher, batch=bool(lead), level_median=3, uniqueness_ratio=15)
                assert meta(r) == [(lead + (3, 10, 21), f64, "cuda")] + [(fl, f64, "cuda")] * 3 + [(px, u32, "cuda")] * 2
            flow = torch.empty(lead + (2, 10, 21), dtype=torch.float64, device="cuda")
            for size in (0, 3, 5):
                assert meta([torch_ops.flow_level_hints(flow, size)]) == [(lead + (2, 20, 42), f64, "cuda")]
            with pytest.raises(ValueError, match="level_median"):
                torch_ops.pyramidal_sgm(I, I, 2, batch=bool(lead), level_median=4)
            with pytest.raises(ValueError, match="level_median"):
                torch_ops.flow_level_hints(flow, 1)
        raw = torch.ops.fsgm.pyramidal_sgm_lm(torch.empty((2, 10, 21), dtype=torch.uint8, device="cuda"),
                                              torch.empty((2, 10, 21), dtype=torch.uint8, device="cuda"), 2, [6, 32, 2, 5, 5, 1, 2, 0], 3, False)
        assert tuple(raw[2].shape) == (0,) and raw[2].dtype == torch.uint32
