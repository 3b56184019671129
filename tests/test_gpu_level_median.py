"""GPU tests of the median between pyramid levels: the kernel on its own on edge values, both pyramid drivers, the warm-plan
sequences and pyramidal_flow_pp, every one bit-exact against the numpy restatement (tests/level_median_restatement.py) composed
from the oracle's single-level matchers.  The restatements are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, _lib  # noqa: E402,F401  (torch first, then the library)
from fsgm_amd import pyramid as _pyramid  # noqa: E402
from tests import edge_inputs as E  # noqa: E402
from tests import flow_pp_restatement as FP  # noqa: E402
from tests import level_median_restatement as LM  # noqa: E402
from tests import ng_runner_up_restatement as NR  # noqa: E402
from tests import runner_up2d_restatement as RU2  # noqa: E402

pytestmark = pytest.mark.gpu
MATCHERS = ("pyd", "ng")
SEED = 11        # chosen on the CPU from the oracle compositions alone: the median changes level 1 of every case that can show it
# (W, H, channels, numPyd): odd sizes (the hint map exceeds the finer image), maps smaller than the window, one level
CASES = [(64, 48, 1, 3), (61, 47, 3, 3), (150, 71, 3, 4), (5, 4, 1, 2), (2, 3, 3, 3), (33, 21, 1, 1)]
COMPARED_ONLY = {(5, 4, 1, 2), (2, 3, 3, 3)}                    # too small for the median to have to change anything
_cache = {}


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)   # (numpy equality: -0.0 == 0.0)


def _pair(W, H, ch, seed=SEED):
    return E.image_pair(E.rng(seed), W, H, ch, seed=seed)


def _want(oracle, matcher, case, s, seed=SEED, swap=False):
    """the restatement of one case: {'levels': flows finest first, 'minC', 'hints': level 1's hint map}; read-only, shared"""
    key = (matcher, case, s, seed, swap)
    if key not in _cache:
        W, H, ch, numPyd = case
        I0, I1 = _pair(W, H, ch, seed)[::-1] if swap else _pair(W, H, ch, seed)
        if matcher == "pyd":
            _, minC, levels, hints = LM.pyramidal_sgm_lm(oracle, I0, I1, numPyd, s)
        else:
            flows, minC, hints = LM.pyramidal_ng_lm(oracle, I0, I1, numPyd, s)
            levels = flows[::-1]
        for a in list(levels) + [minC, hints]:
            a.setflags(write=False)
        _cache[key] = {"levels": levels, "minC": minC, "hints": hints}
    return _cache[key]


def _run(matcher, I0, I1, numPyd, **kw):
    """(flow of level 1, [flow per level, finest first], minC, ...) of either one-shot call"""
    if matcher == "pyd":
        return fsgm_amd.pyramidal_sgm(I0, I1, numPyd, **kw)
    r = fsgm_amd.pyramidal_sgm_ng(I0, I1, numPyd, **kw)
    return (r[0], r[1][::-1]) + tuple(r[2:])


def _plan(matcher, W, H, ch, numPyd, batch=1):
    cls = fsgm_amd.PyramidPlan if matcher == "pyd" else fsgm_amd.NgPyramidPlan
    return cls(W, H, ch, numPyd, batch=batch)


def _check_run(got, want, what):
    np.testing.assert_array_equal(got[0], want["levels"][0], err_msg=what + " level-1 flow")
    np.testing.assert_array_equal(got[2], want["minC"], err_msg=what + " minC")
    assert len(got[1]) == len(want["levels"])
    for l, (a, b) in enumerate(zip(got[1], want["levels"])):
        np.testing.assert_array_equal(a, b, err_msg=f"{what} flow of level {l + 1}")


def _check_plan(plan, want, what):
    for l, w in enumerate(want["levels"]):
        flow, minC = plan.download(l + 1)
        np.testing.assert_array_equal(flow, w, err_msg=f"{what} download({l + 1})")
    np.testing.assert_array_equal(plan.download(1)[1], want["minC"], err_msg=what + " minC")


# ---------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1), (2, 3), (63, 4), (64, 4), (65, 5), (130, 9)])
def test_the_kernel_on_edge_values(gpu_lib, W, H, frames):
    flows = E.vmf_flows(E.rng(900 + 7 * W + H + frames), W, H, frames, 2)
    nans = np.full((1, 2, H, W), np.nan)
    for s in (3, 5):
        got = fsgm_amd.flow_level_hints(flows, s)
        assert got.shape == (frames, 2, 2 * H, 2 * W)
        for f in range(frames):
            _same(got[f], LM.level_hints(flows[f], s), f"{W}x{H} s={s} frame {f}")
        _same(fsgm_amd.flow_level_hints(flows[0], s), got[0], "one flow without the leading dimension")
        _same(fsgm_amd.flow_level_hints(nans, s)[0], LM.level_hints(nans[0], s), f"{W}x{H} s={s} all NaN")
    got = fsgm_amd.flow_level_hints(flows, 0)
    _same(got, 2.0 * np.repeat(np.repeat(flows, 2, axis=2), 2, axis=3), "size 0 is 2 * repeat")


# ---------------------------------------------------------------------------------------------- the drivers
@pytest.mark.parametrize("s", [3, 5])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("matcher", MATCHERS)
def test_drivers_against_the_restatement(gpu_lib, oracle, matcher, case, s):
    W, H, ch, numPyd = case
    I0, I1 = _pair(W, H, ch)
    want = _want(oracle, matcher, case, s)
    if numPyd >= 2 and case not in COMPARED_ONLY:                # the comparison below is not vacuous: the median matters here
        off = _want(oracle, matcher, case, 0)
        assert (want["levels"][0] != off["levels"][0]).any(), "the restatement with the median equals the one without it in level 1"
    _check_run(_run(matcher, I0, I1, numPyd, level_median=s), want, f"{matcher} one-shot")
    with _plan(matcher, W, H, ch, numPyd) as plan:
        plan.upload(I0, I1)
        plan.set_level_median(s)
        plan.run()
        _check_plan(plan, want, f"{matcher} plan")               # download(l) is mvPyd{l}: the unfiltered flow of every level
        assert plan._call("set_level_median", 4) == 1 and "level_median" in plan.lib.fsgm_last_error().decode()


@pytest.mark.parametrize("matcher", MATCHERS)
def test_no_ops_equal_the_plain_call(gpu_lib, matcher):
    lib = _lib.load()
    for case in ((33, 21, 1, 1), (61, 47, 3, 3)):
        W, H, ch, numPyd = case
        I0, I1 = _pair(W, H, ch)
        plain = _run(matcher, I0, I1, numPyd)
        if numPyd == 1:
            for s in (3, 5):
                got = _run(matcher, I0, I1, numPyd, level_median=s)
                _check_run(got, {"levels": plain[1], "minC": plain[2]}, f"numPyd 1, s={s}")
        # level_median 0 through the _lm entry point itself
        fn, default = ((lib.fsgm_pyramidal_sgm_host_lm, lib.fsgm_pyramid_params_default) if matcher == "pyd" else
                       (lib.fsgm_pyramidal_sgm_ng_host_lm, lib.fsgm_ng_pyramid_params_default))
        prm = default()
        prm.numPyd = numPyd
        mv, minC = np.empty((2, H, W)), np.empty((H, W), np.uint32)
        assert fn(_lib.ptr(I0), _lib.ptr(I1), W, H, ch, C.byref(prm), 0, _lib.ptr(mv), _lib.ptr(minC), None, None) == 0
        np.testing.assert_array_equal(mv, plain[0])
        np.testing.assert_array_equal(minC, plain[2])


@pytest.mark.parametrize("matcher", MATCHERS)
def test_the_switch_toggles_on_one_plan(gpu_lib, oracle, matcher):
    case = (61, 47, 3, 3)
    W, H, ch, numPyd = case
    I0, I1 = _pair(W, H, ch)
    with _plan(matcher, W, H, ch, numPyd) as plan:
        plan.upload(I0, I1)
        for s in (3, 0, 5, 3):
            plan.set_level_median(s)
            plan.run()
            _check_plan(plan, _want(oracle, matcher, case, s), f"{matcher} after switching to {s}")


@pytest.mark.parametrize("matcher", MATCHERS)
def test_the_cached_plans_keep_apart(gpu_lib, oracle, matcher):
    case = (64, 48, 1, 3)
    W, H, ch, numPyd = case
    I0, I1 = _pair(W, H, ch)
    for s in (0, 3, 0, 5, 3, 0):
        got = _run(matcher, I0, I1, numPyd, level_median=s) if s else _run(matcher, I0, I1, numPyd)
        _check_run(got, _want(oracle, matcher, case, s), f"{matcher} one-shot with {s}")


@pytest.mark.parametrize("matcher", MATCHERS)
def test_a_batch_of_three_equals_the_single_pairs(gpu_lib, matcher):
    W, H, ch, numPyd = 61, 47, 1, 3
    pairs = [_pair(W, H, ch, seed) for seed in (11, 12, 13)]
    with _plan(matcher, W, H, ch, numPyd, batch=3) as plan:
        for f, (I0, I1) in enumerate(pairs):
            plan.upload(I0, I1, frame=f)
        plan.set_level_median(3)
        plan.run()
        for f, (I0, I1) in enumerate(pairs):
            one = _run(matcher, I0, I1, numPyd, level_median=3)
            for l in range(numPyd):
                np.testing.assert_array_equal(plan.download(l + 1, frame=f)[0], one[1][l], err_msg=f"frame {f} level {l + 1}")
            np.testing.assert_array_equal(plan.download(1, frame=f)[1], one[2])


def _level1_runner_up(oracle, matcher, g0, g1, hints):
    """(minC, minC2) of level 1 from the restatement's hints: the single-level oracle's volumes through the runner-up rules"""
    hints = np.ascontiguousarray(hints)
    if matcher == "pyd":
        _, mc, _, _, S = oracle.calc_pyd_cost_sgm(g0, g1, hints, 5, 5, 2, 1, 6, 32, 1, 2, 0, want_volumes=True)
        return mc, RU2.runner_up2d(S, 11, 11)[2]
    mc, _, Cc, S = oracle.calc_pyd_cost_sgm_ng(g0, g1, hints, 1, 2, 0, 6, 32, want_volumes=True)
    return mc, NR.ng_runner_up_of_volumes(Cc, S)[2]


@pytest.mark.parametrize("matcher", MATCHERS)
def test_with_the_runner_up_cost(gpu_lib, oracle, matcher):
    case = (64, 48, 1, 3)
    W, H, ch, numPyd = case
    I0, I1 = _pair(W, H, ch)
    want = _want(oracle, matcher, case, 3)
    mc, want2 = _level1_runner_up(oracle, matcher, I0, I1, want["hints"])
    np.testing.assert_array_equal(mc, want["minC"])
    got = _run(matcher, I0, I1, numPyd, level_median=3, runner_up=True)
    assert len(got) == 4
    _check_run(got, want, f"{matcher} with runner_up")
    np.testing.assert_array_equal(got[3], want2)
    assert len(_run(matcher, I0, I1, numPyd, level_median=3)) == 3


# ---------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("ratio", [None, 15])
@pytest.mark.parametrize("matcher", MATCHERS)
def test_flow_pp_with_the_median(gpu_lib, oracle, matcher, ratio):
    case = (61, 47, 3, 3)
    W, H, ch, numPyd = case
    I0, I1 = _pair(W, H, ch)
    f, b = _want(oracle, matcher, case, 3), _want(oracle, matcher, case, 3, swap=True)
    fwd, bwd = f["levels"][0], b["levels"][0]
    assert (fwd != _want(oracle, matcher, case, 0)["levels"][0]).any()
    kw = {} if ratio is None else {"uniqueness_ratio": ratio}
    got = fsgm_amd.pyramidal_flow_pp(I0, I1, numPyd, matcher, level_median=3, **kw)
    assert len(got) == (5 if ratio is None else 6)
    _same(got[2], fwd, "flow_fwd is the raw level-1 flow of the forward run")
    _same(got[3], bwd, "flow_bwd is the raw level-1 flow of the backward run")
    np.testing.assert_array_equal(got[4], f["minC"])
    if ratio is None:
        want_pp, want_c, _ = FP.chain(fwd, bwd)
    else:
        g0, g1 = oracle.rgb2gray(I0), oracle.rgb2gray(I1)
        cf, c2f = _level1_runner_up(oracle, matcher, g0, g1, f["hints"])
        cb, c2b = _level1_runner_up(oracle, matcher, g1, g0, b["hints"])
        np.testing.assert_array_equal(got[5], c2f)
        want_pp, want_c, _ = NR.flow_pp_u(fwd, bwd, cf, c2f, cb, c2b, ratio)
    _same(got[0], want_pp, "flow_pp")
    _same(got[1], want_c, "flow_checked")
    plain = fsgm_amd.pyramidal_flow_pp(I0, I1, numPyd, matcher, **kw)          # the plan without the median is still its own
    _same(plain[2], _want(oracle, matcher, case, 0)["levels"][0], "the plain pipeline after the median one")
    both = fsgm_amd.pyramidal_flow_pp(np.stack([I0, I1]), np.stack([I1, I0]), numPyd, matcher, level_median=3, **kw)
    for g, w in zip(both, got):
        _same(g[0], w, "frame 0 of a batch of two")
    _same(both[2][1], bwd, "frame 1 of the batch runs the swapped pair")


def test_python_refusals_on_the_device_box(gpu_lib):
    I0, I1 = _pair(32, 24, 1)
    with pytest.raises(ValueError, match="level_median"):
        fsgm_amd.pyramidal_sgm_batch([(I0, I1)], 2, devices=(0,), level_median=3)
    with fsgm_amd.PyramidPlan(32, 24, 1, 2) as plan:
        with pytest.raises(ValueError, match="level_median"):
            plan.set_level_median(4)
    lib = _lib.load()
    prm = _pyramid.flow_pp_params(lib, "pyd", 2, 0, 0, {})
    pp = np.zeros((3, 24, 32))
    p = _lib.ptr
    assert lib.fsgm_pyramidal_flow_pp_host_lm(1, p(I0), p(I1), 32, 24, 1, C.byref(prm), 15, 3, p(pp), None, None, None, None, None) == 1
    assert "minC2" in lib.fsgm_last_error().decode() and not pp.any()
