"""CPU tests of the neighbour-guided matcher's runner-up cost and of the pyramids' and the pipeline's new forms: the numpy
restatement on hand-built cases with known answers, every refusal of the new entry points that answers before a device is
touched, the Python signatures, and the new torch ops' schemas and fake implementations."""
import ctypes as C
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, ng as _ng, pyramid as _pyramid  # noqa: E402
from tests import ng_runner_up_restatement as NR  # noqa: E402

INVALID = 1
NONE = NR.NO_RUNNER_UP
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first


def _ru(mv, S):
    mv = np.asarray(mv, np.int64)
    return NR.ng_runner_up(mv[:, 0], mv[:, 1], np.asarray(S, np.uint32))


# ---- the rule on hand-built cases ----
def test_all_candidates_equal_have_no_runner_up():
    best, c, c2 = _ru([(3, -2)] * 9, [7, 7, 5, 9, 5, 7, 7, 7, 7])
    assert (best, c, c2) == (2, 5, NONE)
    # a ring of distance 1 around the winner is the winner's own minimum, not a competitor
    ring = [(x, y) for x in (-1, 0, 1) for y in (-1, 0, 1)]
    assert _ru(ring, [4, 4, 4, 4, 1, 4, 4, 4, 4])[2] == NONE


def test_one_far_candidate():
    mv = [(0, 0), (1, 1), (0, 2), (-1, 0), (5, 5)]
    assert _ru(mv, [3, 9, 8, 2, 40]) == (3, 2, 8)                # winner (-1, 0): (1, 1) is two away in x, (0, 2) in y, (0, 0) is not
    assert _ru(mv, [3, 9, 8, 20, 40]) == (0, 3, 8)               # winner (0, 0): (0, 2) and (5, 5)
    assert _ru(mv[:2] + mv[3:4], [3, 9, 2])[2] == 9
    assert _ru([(0, 0), (0, 1), (1, 0)], [3, 9, 2])[2] == NONE


def test_repeats_of_the_winners_vector_never_compete():
    # index 1 wins the tie with index 4 (first minimum); the repeats of its vector at 3 and 4 carry smaller-or-equal sums than
    # the only far candidate and are skipped all the same: the distance is between vectors, not list indices
    mv = [(2, 2), (0, 0), (4, 0), (0, 0), (0, 0), (1, -1)]
    S = [9, 1, 30, 2, 1, 3]
    assert _ru(mv, S) == (1, 1, 9)
    assert _ru(mv[1:], S[1:]) == (0, 1, 30)
    # list neighbours (|d - best| = 1) with far vectors do compete
    assert _ru([(0, 0), (9, 9)], [1, 2]) == (0, 1, 2)


def test_vectors_near_two_to_the_thirty_and_thirty_one():
    big = 2 ** 30
    assert _ru([(big - 1, 0), (big, 0), (big + 1, 0)], [5, 1, 7])[2] == NONE
    assert _ru([(big - 1, 0), (big + 1, 0), (-big, 0)], [5, 1, 7]) == (1, 1, 5)
    lo, hi = -2 ** 31, 2 ** 31 - 1                              # a 32-bit difference would wrap to 1 here
    assert _ru([(lo, 0), (hi, 0)], [1, 6]) == (0, 1, 6)
    assert _ru([(0, hi), (0, lo), (0, hi - 1)], [4, 9, 2]) == (2, 2, 9)


def test_restatement_on_random_lists_equals_a_plain_loop():
    rng = np.random.default_rng(5)
    mvx, mvy = rng.integers(-3, 4, (50, 27)), rng.integers(-3, 4, (50, 27))
    S = rng.integers(0, 12, (50, 27)).astype(np.uint32)
    best, c, c2 = NR.ng_runner_up(mvx, mvy, S)
    for p in range(50):
        b = min(range(27), key=lambda d: (int(S[p, d]), d))
        far = [int(S[p, d]) for d in range(27) if max(abs(mvx[p, d] - mvx[p, b]), abs(mvy[p, d] - mvy[p, b])) >= 2]
        assert (best[p], c[p], c2[p]) == (b, S[p, b], min(far) if far else NONE)
    assert c2.dtype == np.uint32


def test_pipeline_restatement_with_ratio_zero_is_the_chain():
    from tests import flow_pp_inputs, flow_pp_restatement as R
    f, b = flow_pp_inputs.flow_pair(21, 13, "general", seed=3)
    c = np.full((13, 21), 10, np.uint32)
    got = NR.flow_pp_u(f, b, c, c, c, c, 0)
    want = R.chain(f, b)
    for g, w in zip(got[:2], want[:2]):
        np.testing.assert_array_equal(np.nan_to_num(g, nan=-1e9), np.nan_to_num(w, nan=-1e9))
    # ratio 100 with equal costs rejects everything: minC2 * 0 < minC * 100
    assert not got[2]["speckle"].all() and np.isnan(NR.flow_pp_u(f, b, c, c, c, c, 100)[1]).all()


# ---- refusals before a device ----
def _err(lib):
    return lib.fsgm_last_error().decode()


def test_single_level_entry_points_refuse_before_any_device():
    lib = _lib.load()
    _ng._bind(lib)
    a, o = _ng.NgIn(), _ng.NgOut()
    assert lib.fsgm_calc_pyd_cost_sgm_ng_host_ru(C.byref(a), C.byref(o), None, 0) == INVALID and "minC2" in _err(lib)
    assert lib.fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(1, C.byref(a), C.byref(o), None, 0) == INVALID and "minC2s" in _err(lib)
    ins, outs = (_ng.NgIn * 2)(), (_ng.NgOut * 2)()
    one_null = (C.c_void_p * 2)(None, FAKE)
    assert lib.fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(2, ins, outs, one_null, 0) == INVALID and "frame 0 has a null minC2" in _err(lib)
    some = (C.c_void_p * 2)(FAKE, FAKE)
    assert lib.fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(0, ins, outs, some, 0) == INVALID
    assert lib.fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(2, ins, outs, some, 0) == INVALID and "null pointer" in _err(lib)
    assert lib.fsgm_calc_pyd_cost_sgm_ng_host_ru(C.byref(a), C.byref(o), FAKE, 0) == INVALID and "null pointer" in _err(lib)


def test_pyramid_entry_points_refuse_before_any_device():
    lib = _lib.load()
    _pyramid._bind(lib)
    _pyramid._bind_ng(lib)
    _pyramid._bind_flow_pp(lib)
    vp, i32 = C.c_void_p, C.c_int32
    lib.fsgm_pyramidal_sgm_device_ru.argtypes = [i32, vp, vp, i32, i32, i32, C.POINTER(_pyramid.PyramidParams), vp, vp, vp, vp, vp]
    lib.fsgm_pyramidal_sgm_ng_device_ru.argtypes = [i32, vp, vp, i32, i32, i32, C.POINTER(_pyramid.NgPyramidParams), vp, vp, vp, vp, vp]
    for default, host, dev, pre in ((lib.fsgm_pyramid_params_default, lib.fsgm_pyramidal_sgm_host_ru, lib.fsgm_pyramidal_sgm_device_ru,
                                     "fsgm_pyramid_plan_"),
                                    (lib.fsgm_ng_pyramid_params_default, lib.fsgm_pyramidal_sgm_ng_host_ru,
                                     lib.fsgm_pyramidal_sgm_ng_device_ru, "fsgm_ng_pyramid_plan_")):
        prm = default()
        assert host(FAKE, FAKE, 8, 4, 1, C.byref(prm), FAKE, FAKE, None, None) == INVALID and "minC2" in _err(lib)
        assert host(FAKE, FAKE, 8, 4, 1, C.byref(prm), FAKE, None, None, None) == INVALID and "minC2" in _err(lib)
        assert host(None, FAKE, 8, 4, 1, C.byref(prm), FAKE, FAKE, FAKE, None) == INVALID and "null" in _err(lib)
        assert dev(1, FAKE, FAKE, 8, 4, 1, C.byref(prm), FAKE, FAKE, None, None, None) == INVALID and "minC2" in _err(lib)
        assert dev(0, FAKE, FAKE, 8, 4, 1, C.byref(prm), FAKE, FAKE, FAKE, None, None) == INVALID and "n_frames" in _err(lib)
        assert getattr(lib, pre + "set_runner_up")(None, 1) == INVALID and "null plan" in _err(lib)
        assert getattr(lib, pre + "download_runner_up")(None, 0, FAKE) == INVALID and "null" in _err(lib)


@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_pipeline_entry_points_refuse_before_any_device(matcher):
    lib = _lib.load()
    prm = _pyramid.flow_pp_params(lib, matcher, 2, 0, 0, {})
    host = lambda ratio=15, m2=FAKE, n=1, I0=FAKE, p=C.byref(prm): lib.fsgm_pyramidal_flow_pp_host_u(              # noqa: E731
        n, I0, FAKE, 8, 4, 1, p, ratio, FAKE, None, None, None, None, m2)
    dev = lambda ratio=15, m2=FAKE, n=1, I0=FAKE, p=C.byref(prm): lib.fsgm_pyramidal_flow_pp_device_u(             # noqa: E731
        n, I0, FAKE, 8, 4, 1, p, ratio, FAKE, None, None, None, None, m2, None, None)
    for fn in (host, dev):
        for ratio in (-1, 101, 1000):
            assert fn(ratio=ratio) == INVALID and "uniqueness_ratio" in _err(lib)
        assert fn(m2=None) == INVALID and "minC2" in _err(lib)
        assert fn(n=0) == INVALID and "n_frames" in _err(lib)
        assert fn(I0=None) == INVALID and "null" in _err(lib)
        assert fn(p=None) == INVALID and "parameters" in _err(lib)
        bad = _pyramid.flow_pp_params(lib, matcher, 2, 0, 0, {})
        bad.fb_thr = -1.0
        assert fn(p=C.byref(bad)) == INVALID and "fb_thr" in _err(lib)
        bad = _pyramid.flow_pp_params(lib, matcher, 2, 64, 0, {})
        assert fn(p=C.byref(bad)) == INVALID and "out of range" in _err(lib)


# ---- Python ----
def test_python_signatures_and_validation():
    for fn in (fsgm_amd.calc_pyd_cost_sgm_ng, fsgm_amd.calc_pyd_cost_sgm_ng_batch, fsgm_amd.pyramidal_sgm, fsgm_amd.pyramidal_sgm_ng,
               torch_ops.pyramidal_sgm, torch_ops.pyramidal_sgm_ng):
        assert inspect.signature(fn).parameters["runner_up"].default is False
    for fn in (fsgm_amd.pyramidal_flow_pp, torch_ops.pyramidal_flow_pp):
        assert inspect.signature(fn).parameters["uniqueness_ratio"].default is None
    for cls in (fsgm_amd.PyramidPlan, fsgm_amd.NgPyramidPlan):
        assert callable(cls.set_runner_up) and callable(cls.download_runner_up)
    I = np.zeros((4, 6), np.uint8)
    for ratio in (-1, 101, 2.5, True, "7"):
        with pytest.raises((ValueError, TypeError), match="uniqueness_ratio|int"):
            fsgm_amd.pyramidal_flow_pp(I, I, 2, uniqueness_ratio=ratio)
    with pytest.raises(ValueError, match="device list"):
        fsgm_amd.calc_pyd_cost_sgm_ng_batch([(I, I, np.zeros((2, 4, 6)))], 1, 2, 0, 6, 32, devices=(0,), runner_up=True)
    with pytest.raises(ValueError, match="out does not match"):
        fsgm_amd.pyramidal_sgm_ng(I, I, 1, runner_up=True, out=(np.zeros((2, 4, 6)), [np.zeros((2, 4, 6))], np.zeros((4, 6), np.uint32)))


# ---- the torch ops ----
def test_schemas():
    sig = "(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params) -> "
    assert str(torch.ops.fsgm.pyramidal_sgm_ru.default._schema) == "fsgm::pyramidal_sgm_ru" + sig + "(Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.fsgm.pyramidal_sgm_ng_ru.default._schema) == "fsgm::pyramidal_sgm_ng_ru" + sig + "(Tensor, Tensor, Tensor, Tensor)"
    pp = "(Tensor I0, Tensor I1, SymInt matcher, SymInt numPyd, SymInt[] params, float[] chain, SymInt median"
    assert str(torch.ops.fsgm.pyramidal_flow_pp_u.default._schema) == (
        "fsgm::pyramidal_flow_pp_u" + pp + ", SymInt uniqueness_ratio) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    # the neighbours are what they were
    assert str(torch.ops.fsgm.pyramidal_sgm.default._schema) == "fsgm::pyramidal_sgm" + sig + "(Tensor, Tensor, Tensor)"
    assert str(torch.ops.fsgm.pyramidal_sgm_ng.default._schema) == "fsgm::pyramidal_sgm_ng" + sig + "(Tensor, Tensor, Tensor)"
    assert str(torch.ops.fsgm.pyramidal_flow_pp.default._schema) == (
        "fsgm::pyramidal_flow_pp" + pp + ") -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")


def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    meta = lambda ts: [(tuple(t.shape), t.dtype, t.device.type) for t in ts]          # noqa: E731
    with FakeTensorMode():
        for lead in ((), (3,)):
            I = torch.empty(lead + (10, 21), dtype=torch.uint8, device="cuda")
            px, fl = lead + (10, 21), lead + (2, 10, 21)
            for fn in (torch_ops.pyramidal_sgm, torch_ops.pyramidal_sgm_ng):
                r = fn(I, I, 2, batch=bool(lead), runner_up=True, return_status=True)
                assert meta(r) == [(fl, torch.float64, "cuda")] + [(px, torch.uint32, "cuda")] * 2 + [((), torch.int32, "cuda")]
                assert len(fn(I, I, 2, batch=bool(lead))) == 2
            for matcher in ("pyd", "ng"):
                r = torch_ops.pyramidal_flow_pp(I, I, 2, matcher, batch=bool(lead), uniqueness_ratio=15)
                assert meta(r) == [(lead + (3, 10, 21), torch.float64, "cuda")] + [(fl, torch.float64, "cuda")] * 3 + [
                    (px, torch.uint32, "cuda")] * 2
                assert len(torch_ops.pyramidal_flow_pp(I, I, 2, matcher, batch=bool(lead))) == 5
            with pytest.raises(ValueError, match="uniqueness_ratio"):
                torch_ops.pyramidal_flow_pp(I, I, 2, batch=bool(lead), uniqueness_ratio=101)
