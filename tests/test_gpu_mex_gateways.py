"""The mexFunction gateways called the way the MATLAB drivers call them, vs the CPU oracle.
epipolar_sgm_of.m:45, pyramidal_sgm.m:50, ng_sgm.m:20."""
import ctypes
import numpy as np
import pytest

from fsgm_amd import synth
from tests import mexharness as mh

pytestmark = pytest.mark.gpu


def test_calc_cost_sgm_gateway_as_epipolar_sgm_of_calls_it(gpu_lib, oracle):
    W, H, D = 96, 64, 64
    I1, I2 = synth.image_pair(W, H, D, seed=3)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=6)
    (bestD, minC), _ = mh.call("calc_cost_sgm", 2, I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    rbd, rmc = oracle.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, 4)      # as shipped: 4 paths
    assert bestD.dtype == np.uint32 and bestD.shape == (H, W)
    np.testing.assert_array_equal(bestD, rbd)
    np.testing.assert_array_equal(minC, rmc)
    outs, _ = mh.call("calc_cost_sgm", 4, I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    assert outs[2].dtype == np.uint8 and not outs[2].any() and outs[3].dtype == np.uint32 and not outs[3].any()
    (only,), _ = mh.call("calc_cost_sgm", 0, I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    np.testing.assert_array_equal(only, rbd)
    # FSGM_EPI_FB_CHECK=1: the commented-out forward-backward check fills outputs 3 and 4
    import os
    os.environ["FSGM_EPI_FB_CHECK"] = "1"
    try:
        outs, _ = mh.call("calc_cost_sgm", 4, I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    finally:
        del os.environ["FSGM_EPI_FB_CHECK"]
    Cv = oracle.epi_cost(I1, I2, D, 0.3, pd0, nd, off)
    idx, _ = oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, 4), W, H, D, 1)
    conf, d2 = oracle.epi_fb_check(idx, pd0, nd, off, 0.3, D + 1)
    np.testing.assert_array_equal(outs[0], rbd)
    np.testing.assert_array_equal(outs[2], conf)
    np.testing.assert_array_equal(outs[3], d2)


def test_calc_pyd_cost_sgm_gateway_as_pyramidal_sgm_calls_it(gpu_lib, oracle):
    W, H = 72, 40
    I1, I2 = synth.image_pair(W, H, 16, seed=8)
    mv = synth.hint_map(W, H, "even", seed=1)
    (minIdx, minC, mvSub), printed = mh.call("calc_pyd_cost_sgm", 3, I1, I2, mv, 5, 5, 2, 1, 6, 32, 1, 2, 0)
    bd, mc, ms = oracle.calc_pyd_cost_sgm(I1, I2, mv, 5, 5, 2, 1, 6, 32, 1, 2, 0)
    assert printed == f"width: {W}, height: {H}, dMax: 121, winRadiusAgg: 2\n"   # calc_pyd_cost_sgm.cpp:491
    assert mvSub.shape == (2, H, W)
    np.testing.assert_array_equal(minIdx, bd)
    np.testing.assert_array_equal(minC, mc)
    np.testing.assert_array_equal(mvSub, ms)


def test_ng_gateways_as_ng_sgm_calls_them(gpu_lib, oracle):
    W, H = 36, 24
    I1, I2 = synth.image_pair(W, H, 16, seed=5)
    hints = np.zeros((2, H, W))                             # ng_sgm.m:17 passes zeros(row, col): one plane only ...
    (minC, flow), printed = mh.call("calc_pyd_cost_sgm_ng", 2, I1, I2, hints, 1, 2, 0, 6, 32)
    rmc, rfl = oracle.calc_pyd_cost_sgm_ng(I1, I2, hints, 1, 2, 0, 6, 32)
    assert "dMax: 81" in printed
    np.testing.assert_array_equal(minC, rmc)
    np.testing.assert_array_equal(flow, rfl)
    # the single-plane W x H hint ng_sgm.m really passes: mvHeight = H/2, lower half = y plane
    (minC1, flow1), _ = mh.call("calc_pyd_cost_sgm_ng", 2, I1, I2, hints[0], 1, 2, 0, 6, 32)
    r1mc, r1fl = oracle.calc_pyd_cost_sgm_ng(I1, I2, hints[0].reshape(2, H // 2, W), 1, 2, 0, 6, 32)
    np.testing.assert_array_equal(minC1, r1mc)
    np.testing.assert_array_equal(flow1, r1fl)

    ctypes.CDLL(None).srand(ctypes.c_uint(1))
    (minC, flow), printed = mh.call("calc_cost_sgm_ng", 2, I1, I2, hints[0], 1, 2, 0, 6, 32)   # ... which this MEX ignores
    rs = oracle.glibc_rand_stream(oracle.sgm_ng_rand_draws(W, H), seed=1)
    rmc, rfl = oracle.calc_cost_sgm_ng(I1, I2, 6, 32, rs)
    assert printed == "dMax : 108\n"
    np.testing.assert_array_equal(minC, rmc)
    np.testing.assert_array_equal(flow, rfl)


def test_fsgm_pyramidal_sgm_gateway_as_a_drop_in_pyramidal_sgm_would_call_it(gpu_lib, oracle):
    """[mv, minC, mvPyd1..3] = fsgm_pyramidal_sgm(permute(I0,[2 1 3]), permute(I1,[2 1 3]), 3) -- the
    argument values of test_psgm.m:33-34 (RGB pair, three levels)."""
    W, H = 85, 47
    g0, g1 = synth.image_pair(W, H, 12, seed=4)
    I0 = np.stack([g0, 255 - g0, g0 // 3 + 80])
    I1 = np.stack([g1, 255 - g1, g1 // 3 + 80])
    outs, _ = mh.call("fsgm_pyramidal_sgm", 5, I0, I1, 3)
    want_mv, want_minC, want_lv = oracle.pyramidal_sgm(I0, I1, 3)
    assert outs[0].shape == (2, H, W) and outs[0].dtype == np.float64 and outs[1].dtype == np.uint32
    np.testing.assert_array_equal(outs[0], want_mv)
    np.testing.assert_array_equal(outs[1], want_minC)
    for l in range(3):
        np.testing.assert_array_equal(outs[2 + l], want_lv[l])
    (only,), _ = mh.call("fsgm_pyramidal_sgm", 1, g0, g1)                       # gray pair, default numPyd = 5
    np.testing.assert_array_equal(only, oracle.pyramidal_sgm(g0, g1, 5)[0])


def test_fsgm_pyramidal_sgm_ng_gateway(gpu_lib, oracle):
    """[flow, minC, flowPyd1..3] = fsgm_pyramidal_sgm_ng(I0p, I1p, 3): the level loop around calc_pyd_cost_sgm_ng
    (BASELINE config 4), against the same composition of the oracle's functions."""
    W, H = 70, 41
    g0, g1 = synth.image_pair(W, H, 8, seed=5)
    I0 = np.stack([g0, 255 - g0, g0 // 3 + 80])
    I1 = np.stack([g1, 255 - g1, g1 // 3 + 80])
    outs, _ = mh.call("fsgm_pyramidal_sgm_ng", 5, I0, I1, 3)
    lv = [(I0, I1)]
    for _ in range(2):
        a, b = lv[-1]
        lv.append((np.stack([oracle.impyramid_reduce(c) for c in a]), np.stack([oracle.impyramid_reduce(c) for c in b])))
    gray = [(oracle.rgb2gray(a), oracle.rgb2gray(b)) for a, b in lv]
    mvPre = np.zeros((2,) + gray[-1][0].shape)
    want = {}
    for l in (3, 2, 1):
        mc, fl = oracle.calc_pyd_cost_sgm_ng(gray[l - 1][0], gray[l - 1][1], mvPre, 1, 2, 0, 6, 32)
        want[l] = fl
        mvPre = np.ascontiguousarray(2.0 * np.repeat(np.repeat(fl, 2, axis=1), 2, axis=2))
    assert outs[0].shape == (2, H, W) and outs[0].dtype == np.float64 and outs[1].dtype == np.uint32
    np.testing.assert_array_equal(outs[0], want[1])
    np.testing.assert_array_equal(outs[1], mc)
    for l in (1, 2, 3):
        np.testing.assert_array_equal(outs[1 + l], want[l])


# ================================================================================================ the whole surface
# Everything below drives the seven gateways over their argument and output surface at small shapes (none above 48 x 32, W != H,
# odd sizes for the pyramids), bit for bit against the CPU oracle (oracle/pyoracle.py; its second restatement
# tests/adaptive_p2_restatement.py for the linear build and adaptive P2, which the oracle's C++ does not have) and, where
# oracle/_ref/ came along with the tree, against the reference's own compiled MEX code on the same argument lists.
import functools                                             # noqa: E402

from oracle import pyoracle as O, pyref                      # noqa: E402
from tests import adaptive_p2_restatement as AP              # noqa: E402
from tests import edge_inputs as EI                          # noqa: E402

SEVEN = ["calc_cost_sgm", "calc_cost_sgm_linear", "calc_pyd_cost_sgm", "calc_pyd_cost_sgm_ng", "calc_cost_sgm_ng",
         "fsgm_pyramidal_sgm", "fsgm_pyramidal_sgm_ng"]
MAX_NLHS = {"calc_cost_sgm": 4, "calc_cost_sgm_linear": 4, "calc_pyd_cost_sgm": 3, "calc_pyd_cost_sgm_ng": 2, "calc_cost_sgm_ng": 2,
            "fsgm_pyramidal_sgm": 5, "fsgm_pyramidal_sgm_ng": 5}                     # the pyramids at numPyd = 3
SHAPES = {"A": (37, 23), "B": (29, 31)}                       # the single-level gateways
PYR_SHAPES = {"A": (45, 31), "B": (33, 27)}                   # the pyramids: odd sizes round up, ceil(size / 2)
D = 16


def _srand1():
    ctypes.CDLL(None).srand(ctypes.c_uint(1))                 # calc_cost_sgm_ng draws its hints from libc rand()


def _run(gw, nlhs, args, want, dims, pre=None):
    """One gateway call checked over its whole output surface.  want / dims: every output the gateway can return and its
    MATLAB dimension list; the call hands back the first max(nlhs, 1) of them.  Checks their number, class, dimension list and
    values, that the inputs are byte-identical afterwards, and that exactly inputs + returned outputs were alive when the call
    came back (a temporary the caller did not ask for is freed)."""
    before = [mh.sent(a) for a in args]
    if pre:
        pre()
    r = mh.call_full(gw, nlhs, *args)
    n = max(nlhs, 1)
    assert len(r.outs) == n
    assert r.live_after == r.live_before + len(args) + n, f"{gw} nlhs={nlhs}: {r.live_after - r.live_before - len(args)} arrays alive, {n} returned"
    assert mh.live_arrays() == r.live_before
    for i in range(n):
        assert r.out_dims[i] == tuple(dims[i]), f"{gw} output {i}: dimensions {r.out_dims[i]}, expected {tuple(dims[i])}"
        assert r.outs[i].dtype == want[i].dtype, f"{gw} output {i}: class {r.outs[i].dtype}, expected {want[i].dtype}"
        np.testing.assert_array_equal(r.outs[i], want[i].reshape(r.outs[i].shape), err_msg=f"{gw} nlhs={nlhs} output {i}")
    for k, (a, b) in enumerate(zip(before, r.inputs_after)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{gw}: input {k} was written"
    return r


# ------------------------------------------------------------------------------------------------ inputs and what the oracle says
@functools.lru_cache(None)
def _epi_frame(seed, kind, W, H):
    I1, I2 = synth.image_pair(W, H, D, seed=seed)
    pd0, nd, off = synth.epi_maps(W, H, kind, seed=seed + 3)
    return I1, I2, pd0, nd, off


def _epi_want(frame, dMax, vMax, P1, P2, paths=4, adaptive=0, fb=0, linear=0):
    """[bestD, minC, conf, bestD2] of calc_cost_sgm (calc_cost_sgm_linear) on one frame; conf and bestD2 are zero unless fb"""
    I1, I2, pd0, nd, off = frame
    H, W = I1.shape
    if linear:
        outs = AP.calc_cost_sgm_linear(I1, I2, dMax, pd0, nd, P1, P2, paths=paths, adaptive=adaptive, fb_check=fb)
    elif adaptive:
        outs = AP.calc_cost_sgm(I1, I2, dMax, vMax, pd0, nd, off, P1, P2, paths=paths, adaptive=1, fb_check=fb)
    else:
        Cv = O.epi_cost(I1, I2, dMax, vMax, pd0, nd, off)
        idx, minC = O.epi_wta(O.epi_aggregate(Cv, P1, P2, paths), W, H, dMax, 1)
        outs = (O.epi_vz_to_disp(idx, off, vMax, dMax + 1), minC) + (tuple(O.epi_fb_check(idx, pd0, nd, off, vMax, dMax + 1)) if fb else ())
        if paths == 4:                                          # the shipped configuration: the oracle's one call says the same
            bd, mc = O.calc_cost_sgm(I1, I2, dMax, vMax, pd0, nd, off, P1, P2, 4)
            assert np.array_equal(bd, outs[0]) and np.array_equal(mc, outs[1])
    outs = list(outs)
    if not fb:
        outs += [np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint32)]
    return [outs[0].astype(np.uint32), outs[1].astype(np.uint32), outs[2].astype(np.uint8), outs[3].astype(np.uint32)]


@functools.lru_cache(None)
def _pair(W, H, seed, rgb=False):
    g0, g1 = synth.image_pair(W, H, 8, seed=seed)
    if rgb:
        return np.stack([g0, 255 - g0, g0 // 3 + 80]), np.stack([g1, 255 - g1, g1 // 3 + 80])
    return g0, g1


@functools.lru_cache(None)
def _hard_pair(W, H, rgb):
    """two unrelated noise images: no candidate stands out and neighbours differ by more than adaptive P2's threshold, so every
    penalty, switch and window size shows in the result"""
    g0, g1 = synth.uniform_u8(6, (H, W)), synth.uniform_u8(13, (H, W))
    if rgb:
        return np.stack([g0, 255 - g0, g0 // 3 + 80]), np.stack([g1, 255 - g1, g1 // 3 + 80])
    return g0, g1


def _pyr_dims(W, H, numPyd):
    return [(W, H, 2), (W, H)] + [(w, h, 2) for (w, h) in O.pyramid_sizes(W, H, numPyd)]


def _pyd_pyramid_want(I0, I1, numPyd, **kw):
    mv, minC, lv = O.pyramidal_sgm(I0, I1, numPyd, **kw)
    return [mv, minC] + list(lv)


def _ng_pyramid_want(I0, I1, numPyd, **kw):
    flows, minC = EI.oracle_pyramidal_ng(O, I0, I1, numPyd, **kw)          # flows: coarsest level first
    return [flows[-1], minC] + flows[::-1]


@functools.lru_cache(None)
def _case(gw, shape="A"):
    """(args, want, dims, pre) of a plain call of the gateway: the reference's argument values, small shapes"""
    if gw.startswith("fsgm_pyramidal"):
        W, H = PYR_SHAPES[shape]
        I0, I1 = _pair(W, H, 4, rgb=(shape == "A"))
        want = (_pyd_pyramid_want if gw == "fsgm_pyramidal_sgm" else _ng_pyramid_want)(I0, I1, 3)
        return (I0, I1, 3), want, _pyr_dims(W, H, 3), None
    W, H = SHAPES[shape]
    if gw in ("calc_cost_sgm", "calc_cost_sgm_linear"):
        fr = _epi_frame(3, "general", W, H)
        return ((fr[0], fr[1], D, 0.3, fr[2], fr[3], fr[4], 6, 64), _epi_want(fr, D, 0.3, 6, 64, linear=gw.endswith("linear")),
                [(W, H)] * 4, None)
    I1, I2 = _pair(W, H, 8)
    if gw == "calc_pyd_cost_sgm":
        mv = synth.hint_map(W, H, "even", seed=1)
        return ((I1, I2, mv, 2, 1, 2, 1, 6, 32, 1, 2, 0), list(O.calc_pyd_cost_sgm(I1, I2, mv, 2, 1, 2, 1, 6, 32, 1, 2, 0)),
                [(W, H), (W, H), (W, H, 2)], None)
    if gw == "calc_pyd_cost_sgm_ng":
        mv = synth.hint_map(W, H, "int", seed=2)
        return (I1, I2, mv, 1, 2, 0, 6, 32), list(O.calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 0, 6, 32)), [(W, H), (W, H, 2)], None
    assert gw == "calc_cost_sgm_ng"
    rs = O.glibc_rand_stream(O.sgm_ng_rand_draws(W, H), seed=1)
    return (I1, I2, np.zeros((H, W)), 1, 2, 0, 6, 32), list(O.calc_cost_sgm_ng(I1, I2, 6, 32, rs)), [(W, H), (W, H, 2)], _srand1


def _with(args, changes):
    a = list(args)
    for k, v in changes.items():
        a[k] = v
    return a


def _ref(name):
    return pyref.available(name)


def _same_as_ref(ref_outs, want, what):
    for i, (a, b) in enumerate(zip(ref_outs, want)):
        np.testing.assert_array_equal(a, b.reshape(a.shape), err_msg=f"the reference's MEX and the oracle differ: {what}, output {i}")


# ------------------------------------------------------------------------------------------------ every output count
@pytest.mark.parametrize("gw,nlhs", [(g, k) for g in SEVEN for k in range(MAX_NLHS[g] + 1)])
def test_every_output_count(gpu_lib, oracle, gw, nlhs):
    args, want, dims, pre = _case(gw)
    _run(gw, nlhs, args, want, dims, pre)


@pytest.mark.parametrize("gw", SEVEN)
def test_shapes_a_b_a_in_one_process(gpu_lib, oracle, gw):
    """cached plans are evicted and reused behind the gateway: the third call gives what the first gave"""
    first = None
    for shape in "ABA":
        args, want, dims, pre = _case(gw, shape)
        r = _run(gw, MAX_NLHS[gw], args, want, dims, pre)
        if first is None:
            first = r
    for a, b in zip(first.outs, r.outs):
        assert a.tobytes() == b.tobytes()


def test_a_refused_call_does_not_spoil_the_next(gpu_lib, oracle):
    args, want, dims, _ = _case("calc_cost_sgm")
    for changes, ident in (({1: np.ascontiguousarray(args[1][:, :-1])}, "fsgm:size"), ({2: 1025}, "fsgm:unsupported")):
        with pytest.raises(mh.MexError) as e:                  # dMax = 1025: the library refuses it before any launch
            mh.call_full("calc_cost_sgm", 4, *_with(args, changes))
        assert e.value.ident == ident and e.value.leaked == 0, str(e.value)
        _run("calc_cost_sgm", 4, args, want, dims)
    args, want, dims, _ = _case("calc_pyd_cost_sgm")
    with pytest.raises(mh.MexError) as e:
        mh.call_full("calc_pyd_cost_sgm", 3, *_with(args, {2: np.zeros((2, args[2].shape[1] - 1, args[2].shape[2]))}))
    assert e.value.ident == "fsgm:size" and e.value.leaked == 0
    _run("calc_pyd_cost_sgm", 3, args, want, dims)
    for gw in ("fsgm_pyramidal_sgm", "fsgm_pyramidal_sgm_ng"):
        args, want, dims, _ = _case(gw)
        with pytest.raises(mh.MexError) as e:
            mh.call_full(gw, 2, *_with(args, {2: 17}))
        assert e.value.ident == "fsgm:range" and e.value.leaked == 0
        _run(gw, 5, args, want, dims)


# ------------------------------------------------------------------------------------------------ conversions
S, I32 = np.float32, np.int32
EPI_CONV = [                                               # (label, arguments as given, (dMax, vMax, P1, P2) as converted)
    ("truncate", {2: 16.7, 7: 6.9, 8: 32.999}, (16, 0.3, 6, 32)),
    ("P1_-0.5", {7: -0.5}, (16, 0.3, 0, 64)),
    ("int32", {2: I32(16), 7: I32(5)}, (16, 0.3, 5, 64)),
    ("single", {2: S(16), 7: S(5.5)}, (16, 0.3, 5, 64)),
    ("vMax_single", {3: S(0.3)}, (16, float(S(0.3)), 6, 64)),
]


@pytest.mark.parametrize("gw", ["calc_cost_sgm", "calc_cost_sgm_linear"])
@pytest.mark.parametrize("case", EPI_CONV, ids=[c[0] for c in EPI_CONV])
def test_epipolar_scalars_convert_like_the_reference(gpu_lib, oracle, gw, case):
    _, changes, (dMax, vMax, P1, P2) = case
    assert float(S(0.3)) != 0.3
    args, _, dims, _ = _case(gw)
    given = _with(args, changes)
    fr = _epi_frame(3, "general", *SHAPES["A"])
    want = _epi_want(fr, dMax, vMax, P1, P2, linear=gw.endswith("linear"))
    _run(gw, 4, given, want, dims)
    if gw == "calc_cost_sgm" and _ref("calc_cost_sgm"):
        ref, _ = pyref.call_calc_cost_sgm(fr[0], fr[1], float(given[2]), float(given[3]), fr[2], fr[3], fr[4], float(given[7]), float(given[8]))
        _same_as_ref(ref, want, case[0])


NAN = float("nan")
PYD_BASE = dict(rX=2, rY=1, rAgg=2, subpixel=1, P1=6, P2=32, diagonal=1, totalPass=2, adaptiveP2=0)
PYD_CONV = [                                               # (label, arguments as given, oracle parameters as converted)
    ("truncate", {7: 6.9, 8: 32.999}, {}),
    ("P1_-0.5", {7: -0.5}, dict(P1=0)),
    ("sub_1.5", {6: 1.5}, dict(subpixel=1)),
    ("sub_0.5", {6: 0.5}, dict(subpixel=0)),
    ("pass_1", {10: 1}, dict(totalPass=1)),
    ("pass_1.9", {10: 1.9}, dict(totalPass=1)),
    ("pass_2", {10: 2}, dict(totalPass=2)),
    ("int32", {3: I32(2), 7: I32(5), 10: I32(1)}, dict(P1=5, totalPass=1)),
    ("single", {4: S(1), 7: S(5.5), 8: S(40.5)}, dict(P1=5, P2=40)),
] + [(f"diag_{v!r}", {9: v}, dict(diagonal=1)) for v in (0.25, -1, NAN, np.bool_(True))] \
  + [(f"diag_{v!r}", {9: v}, dict(diagonal=0)) for v in (0, -0.0, np.bool_(False))] \
  + [(f"adaptive_{v!r}", {11: v}, dict(adaptiveP2=1)) for v in (0.25, -1, NAN, np.bool_(True))] \
  + [(f"adaptive_{v!r}", {11: v}, dict(adaptiveP2=0)) for v in (0, -0.0)]


@functools.lru_cache(None)
def _pyd_want(items):
    args, _, _, _ = _case("calc_pyd_cost_sgm")
    p = dict(PYD_BASE, **dict(items))
    return list(O.calc_pyd_cost_sgm(args[0], args[1], args[2], p["rX"], p["rY"], p["rAgg"], p["subpixel"], p["P1"], p["P2"], p["diagonal"],
                                    p["totalPass"], p["adaptiveP2"]))


@pytest.mark.parametrize("case", PYD_CONV, ids=[c[0] for c in PYD_CONV])
def test_calc_pyd_cost_sgm_scalars_convert_like_the_reference(gpu_lib, oracle, case):
    """int arguments truncate (int x = mxGetScalar(..)), the two bool arguments are != 0 (NaN and logical(1) included)"""
    label, changes, conv = case
    args, base_want, dims, _ = _case("calc_pyd_cost_sgm")
    want = _pyd_want(tuple(sorted(conv.items())))
    if dict(PYD_BASE, **conv) != PYD_BASE:
        assert any(not np.array_equal(a, b) for a, b in zip(want, base_want)), "the converted value changes nothing at this shape"
    given = _with(args, changes)
    _run("calc_pyd_cost_sgm", 3, given, want, dims)
    if _ref("calc_pyd_cost_sgm"):
        ref, _ = pyref.call_calc_pyd_cost_sgm(args[0], args[1], args[2], *[float(v) for v in given[3:]])
        _same_as_ref(ref, want, label)


NG_CONV = [                                                # (label, arguments as given, (half, aggSize, sub, P1, P2) as converted)
    ("truncate", {3: 1.9, 4: 3.9, 6: 6.9, 7: 32.999}, (1, 3, 0, 6, 32)),
    ("P1_-0.5", {6: -0.5}, (1, 2, 0, 0, 32)),
    ("sub_1.5", {5: 1.5}, (1, 2, 1, 6, 32)),
    ("sub_0.5", {5: 0.5}, (1, 2, 0, 6, 32)),
    ("int32", {3: I32(0), 4: I32(4), 6: I32(5)}, (0, 4, 0, 5, 32)),
    ("single", {3: S(1.5), 5: S(1), 7: S(40.5)}, (1, 2, 1, 6, 40)),
    ("logical_sub", {5: np.bool_(True)}, (1, 2, 1, 6, 32)),
]


@pytest.mark.parametrize("case", NG_CONV, ids=[c[0] for c in NG_CONV])
def test_calc_pyd_cost_sgm_ng_scalars_convert_like_the_reference(gpu_lib, oracle, case):
    label, changes, conv = case
    args, _, dims, _ = _case("calc_pyd_cost_sgm_ng")
    want = list(O.calc_pyd_cost_sgm_ng(args[0], args[1], args[2], *conv))
    given = _with(args, changes)
    _run("calc_pyd_cost_sgm_ng", 2, given, want, dims)
    if _ref("calc_pyd_cost_sgm_ng"):
        ref, _ = pyref.call_calc_pyd_cost_sgm_ng(args[0], args[1], args[2], *[float(v) for v in given[3:]])
        _same_as_ref(ref, want, label)


def test_calc_cost_sgm_ng_converts_p1_p2_and_only_checks_what_it_does_not_use(gpu_lib, oracle):
    args, want, dims, pre = _case("calc_cost_sgm_ng")
    for changes in ({6: 6.9, 7: 32.999}, {6: I32(6), 7: S(32.5)},
                    {2: np.full((1, 1), 7.5), 3: S(7), 4: I32(9), 5: np.bool_(True)}):     # arguments 3..6: any values
        _run("calc_cost_sgm_ng", 2, _with(args, changes), want, dims, pre)
    W, H = SHAPES["A"]
    rs = O.glibc_rand_stream(O.sgm_ng_rand_draws(W, H), seed=1)
    want0 = list(O.calc_cost_sgm_ng(args[0], args[1], 0, 32, rs))
    _run("calc_cost_sgm_ng", 2, _with(args, {6: -0.5}), want0, dims, pre)
    if _ref("calc_cost_sgm_ng"):
        _same_as_ref(pyref.call_calc_cost_sgm_ng(args[0], args[1], 6.9, 32.999, seed=1)[0], want, "P1 = 6.9, P2 = 32.999")
        _same_as_ref(pyref.call_calc_cost_sgm_ng(args[0], args[1], -0.5, 32, seed=1)[0], want0, "P1 = -0.5")


@pytest.mark.parametrize("gw", ["fsgm_pyramidal_sgm", "fsgm_pyramidal_sgm_ng"])
@pytest.mark.parametrize("numPyd", [I32(2), S(3), np.uint8(2)], ids=["int32_2", "single_3", "uint8_2"])
def test_pyramid_level_count_of_any_numeric_class(gpu_lib, oracle, gw, numPyd):
    W, H = PYR_SHAPES["B"]
    I0, I1 = _pair(W, H, 4)
    n = int(numPyd)
    want = (_pyd_pyramid_want if gw == "fsgm_pyramidal_sgm" else _ng_pyramid_want)(I0, I1, n)
    _run(gw, 2 + n, (I0, I1, numPyd), want, _pyr_dims(W, H, n))


# ------------------------------------------------------------------------------------------------ hint maps
@pytest.mark.parametrize("kind", ["general", "int"])
@pytest.mark.parametrize("grow", [(3, 2), (0, 0)], ids=["W+3_H+2", "W_H"])
@pytest.mark.parametrize("gw", ["calc_pyd_cost_sgm", "calc_pyd_cost_sgm_ng"])
def test_hint_maps_larger_than_the_image(gpu_lib, oracle, gw, grow, kind):
    """mvWidth = mxGetM, mvHeight = mxGetN / 2: the y plane starts mvW * mvH doubles in, rows are mvW apart"""
    W, H = SHAPES["A"]
    args, _, dims, _ = _case(gw)
    mv = synth.hint_map(W + grow[0], H + grow[1], kind, seed=5)
    if gw == "calc_pyd_cost_sgm":
        want = list(O.calc_pyd_cost_sgm(args[0], args[1], mv, 2, 1, 2, 1, 6, 32, 1, 2, 0))
    else:
        want = list(O.calc_pyd_cost_sgm_ng(args[0], args[1], mv, 1, 2, 0, 6, 32))
    _run(gw, MAX_NLHS[gw], _with(args, {2: mv}), want, dims)
    if _ref(gw):
        call = pyref.call_calc_pyd_cost_sgm if gw == "calc_pyd_cost_sgm" else pyref.call_calc_pyd_cost_sgm_ng
        _same_as_ref(call(args[0], args[1], mv, *[float(v) for v in args[3:]])[0], want, f"{grow} {kind}")


@pytest.mark.parametrize("H", [24, 23], ids=["H_even", "H_odd"])
def test_the_one_plane_hint_of_ng_sgm(gpu_lib, oracle, H):
    """ng_sgm.m:17 hands calc_pyd_cost_sgm_ng one W x H plane.  mvHeight = floor(H / 2): the first W * mvHeight doubles are the
    x plane, the next W * mvHeight the y plane, and with H odd the last column of the array is not read -- the reference's
    own arithmetic (calc_pyd_cost_sgm_ng.cpp:501-502), pinned here for both parities."""
    W = 37
    I1, I2 = _pair(W, H, 8)
    plane = synth.hint_map(W, H, "int", seed=9)[0]
    mvH = H // 2
    as_read = np.ascontiguousarray(plane.reshape(-1)[:2 * mvH * W].reshape(2, mvH, W))
    want = list(O.calc_pyd_cost_sgm_ng(I1, I2, as_read, 1, 2, 0, 6, 32))
    assert not np.array_equal(want[1], O.calc_pyd_cost_sgm_ng(I1, I2, np.zeros((2, mvH, W)), 1, 2, 0, 6, 32)[1])   # the hints matter
    _run("calc_pyd_cost_sgm_ng", 2, (I1, I2, plane, 1, 2, 0, 6, 32), want, [(W, H), (W, H, 2)])
    if _ref("calc_pyd_cost_sgm_ng"):
        _same_as_ref(pyref.call_calc_pyd_cost_sgm_ng(I1, I2, plane, 1, 2, 0, 6, 32)[0], want, f"one plane, H = {H}")


# ------------------------------------------------------------------------------------------------ calc_cost_sgm_linear, environment
@pytest.mark.parametrize("env,kw", [({"FSGM_EPI_PATHS": "8"}, dict(paths=8)), ({"FSGM_EPI_FB_CHECK": "1"}, dict(fb=1)),
                                    ({"FSGM_EPI_PATHS": "8", "FSGM_EPI_FB_CHECK": "1"}, dict(paths=8, fb=1)),
                                    ({"FSGM_EPI_ADAPTIVE_P2": "1"}, dict(adaptive=1))], ids=["paths8", "fb", "paths8_fb", "adaptive"])
@pytest.mark.parametrize("gw", ["calc_cost_sgm", "calc_cost_sgm_linear"])
def test_epipolar_environment_switches(gpu_lib, oracle, monkeypatch, gw, env, kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args, base_want, dims, _ = _case(gw)
    want = _epi_want(_epi_frame(3, "general", *SHAPES["A"]), D, 0.3, 6, 64, linear=gw.endswith("linear"), **kw)
    assert any(not np.array_equal(a, b) for a, b in zip(want, base_want))
    for nlhs in range(5):
        _run(gw, nlhs, args, want, dims)


# ------------------------------------------------------------------------------------------------ calc_cost_sgm's batch form
BATCH_FRAMES = ((3, "general"), (11, "radial"), (7, "axis"))         # three different images and geometries


@functools.lru_cache(None)
def _batch(n):
    W, H = SHAPES["A"]
    fr = [_epi_frame(seed, kind, W, H) for seed, kind in BATCH_FRAMES[:n]]
    stack = lambda k: np.ascontiguousarray(np.stack([f[k] for f in fr]))                     # noqa: E731
    return fr, (stack(0), stack(1), D, 0.3, stack(2), stack(3), stack(4), 6, 64)


@functools.lru_cache(None)
def _batch_want(n, items):
    fr, _ = _batch(n)
    per = [_epi_want(f, D, 0.3, 6, 64, **dict(items)) for f in fr]
    return per, [np.ascontiguousarray(np.stack([p[i] for p in per])) for i in range(4)]


BATCH_ENVS = [({}, {}), ({"FSGM_EPI_FB_CHECK": "1"}, dict(fb=1)), ({"FSGM_EPI_PATHS": "8"}, dict(paths=8)),
              ({"FSGM_EPI_ADAPTIVE_P2": "1"}, dict(adaptive=1)), ({"FSGM_DEVICES": "0,0"}, {}),
              ({"FSGM_DEVICES": "0,0", "FSGM_EPI_FB_CHECK": "1", "FSGM_EPI_PATHS": "8"}, dict(fb=1, paths=8))]


@pytest.mark.parametrize("env,kw", BATCH_ENVS, ids=["plain", "fb", "paths8", "adaptive", "devices_0,0", "devices_fb_paths8"])
def test_batch_of_three_frames(gpu_lib, oracle, monkeypatch, env, kw):
    """W x H x 3 inputs: every output count, every frame equal to the oracle and to the 2-D call of that frame"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W, H = SHAPES["A"]
    fr, args = _batch(3)
    per, want = _batch_want(3, tuple(sorted(kw.items())))
    for nlhs in range(5):
        _run("calc_cost_sgm", nlhs, args, want, [(W, H, 3)] * 4)
    monkeypatch.delenv("FSGM_DEVICES", raising=False)
    for f, w in zip(fr, per):
        _run("calc_cost_sgm", 4, (f[0], f[1], D, 0.3, f[2], f[3], f[4], 6, 64), w, [(W, H)] * 4)


@pytest.mark.parametrize("fb", [0, 1])
def test_batch_of_one_frame_built_as_w_h_1(gpu_lib, oracle, monkeypatch, fb):
    if fb:
        monkeypatch.setenv("FSGM_EPI_FB_CHECK", "1")
    W, H = SHAPES["A"]
    f = _epi_frame(3, "general", W, H)
    args = (mh.Arr(f[0], (W, H, 1)), mh.Arr(f[1], (W, H, 1)), D, 0.3, mh.Arr(f[2], (W, H, 2, 1)), mh.Arr(f[3], (W, H, 2, 1)),
            mh.Arr(f[4], (W, H, 1)), 6, 64)
    want = _epi_want(f, D, 0.3, 6, 64, fb=fb)
    for nlhs in range(5):
        _run("calc_cost_sgm", nlhs, args, want, [(W, H)] * 4)      # one plane: the outputs are 2-D


# ------------------------------------------------------------------------------------------------ the pyramids' environment
PYD_ENV = {"FSGM_PYD_P1": ("9", dict(P1=9)), "FSGM_PYD_P2": ("48", dict(P2=48)), "FSGM_PYD_AGG": ("1", dict(aggHalfWinSize=1)),
           "FSGM_PYD_VER": ("2", dict(ver=2)), "FSGM_PYD_HOR": ("4", dict(hor=4)), "FSGM_PYD_ADAPTIVE_P2": ("1", dict(adaptiveP2=1))}
NG_ENV = {"FSGM_NG_P1": ("9", dict(P1=9)), "FSGM_NG_P2": ("48", dict(P2=48)), "FSGM_NG_HALF_SEARCH": ("0", dict(half=0)),
          "FSGM_NG_AGG_SIZE": ("4", dict(agg=4)), "FSGM_NG_SUBPIXEL": ("1", dict(sub=1))}
INPUTS = [(False, 2), (True, 3)]                              # (RGB, numPyd)


@functools.lru_cache(None)
def _pyramid_want(gw, rgb, numPyd, items):
    W, H = PYR_SHAPES["A"]
    I0, I1 = _hard_pair(W, H, rgb)
    return (_pyd_pyramid_want if gw == "fsgm_pyramidal_sgm" else _ng_pyramid_want)(I0, I1, numPyd, **dict(items))


def _pyramid_env_case(monkeypatch, gw, env, kw, rgb, numPyd, differs=True):
    table = PYD_ENV if gw == "fsgm_pyramidal_sgm" else NG_ENV
    for k in table:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W, H = PYR_SHAPES["A"]
    I0, I1 = _hard_pair(W, H, rgb)
    want = _pyramid_want(gw, rgb, numPyd, tuple(sorted(kw.items())))
    if differs:                                              # the override is visible in what the oracle computes
        base = _pyramid_want(gw, rgb, numPyd, ())
        assert any(not np.array_equal(a, b) for a, b in zip(want, base)), f"{env} changes nothing at this shape"
    _run(gw, 2 + numPyd, (I0, I1, numPyd), want, _pyr_dims(W, H, numPyd))


@pytest.mark.parametrize("rgb,numPyd", INPUTS, ids=["gray2", "rgb3"])
@pytest.mark.parametrize("var", list(PYD_ENV))
def test_fsgm_pyramidal_sgm_environment_one_at_a_time(gpu_lib, oracle, monkeypatch, var, rgb, numPyd):
    _pyramid_env_case(monkeypatch, "fsgm_pyramidal_sgm", {var: PYD_ENV[var][0]}, PYD_ENV[var][1], rgb, numPyd)


@pytest.mark.parametrize("rgb,numPyd", INPUTS, ids=["gray2", "rgb3"])
@pytest.mark.parametrize("var", list(NG_ENV))
def test_fsgm_pyramidal_sgm_ng_environment_one_at_a_time(gpu_lib, oracle, monkeypatch, var, rgb, numPyd):
    _pyramid_env_case(monkeypatch, "fsgm_pyramidal_sgm_ng", {var: NG_ENV[var][0]}, NG_ENV[var][1], rgb, numPyd)


@pytest.mark.parametrize("rgb", [False, True], ids=["gray", "rgb"])
@pytest.mark.parametrize("numPyd", [2, 3])
@pytest.mark.parametrize("gw", ["fsgm_pyramidal_sgm", "fsgm_pyramidal_sgm_ng"])
def test_pyramid_environment_all_together(gpu_lib, oracle, monkeypatch, gw, numPyd, rgb):
    table = PYD_ENV if gw == "fsgm_pyramidal_sgm" else NG_ENV
    env = {k: v[0] for k, v in table.items()}
    kw = {}
    for v in table.values():
        kw.update(v[1])
    if gw == "fsgm_pyramidal_sgm_ng":
        env["FSGM_NG_HALF_SEARCH"], kw["half"] = "2", 2       # 9 * 25 candidates; 0 (9 candidates) is the one-at-a-time case
    _pyramid_env_case(monkeypatch, gw, env, kw, rgb, numPyd)


@pytest.mark.parametrize("gw,var,name", [("fsgm_pyramidal_sgm", "FSGM_PYD_P1", "P1"), ("fsgm_pyramidal_sgm_ng", "FSGM_NG_P1", "P1"),
                                         ("fsgm_pyramidal_sgm", "FSGM_PYD_HOR", "hor"), ("fsgm_pyramidal_sgm_ng", "FSGM_NG_AGG_SIZE", "agg")])
def test_pyramid_environment_empty_and_non_numeric_values(gpu_lib, oracle, monkeypatch, gw, var, name):
    """VAR= is the default; anything else is what atoi gives: "7x" is 7, "abc" is 0"""
    _pyramid_env_case(monkeypatch, gw, {var: ""}, {}, False, 2, differs=False)
    _pyramid_env_case(monkeypatch, gw, {var: "7x"}, {name: 7}, False, 2)
    _pyramid_env_case(monkeypatch, gw, {var: "abc"}, {name: 0}, False, 2)
