"""The mexFunction gateways (the reference's four MEX names, calc_cost_sgm's linear build and the two pyramidal drivers): they load,
export mexFunction, and validate arguments loudly (no GPU needed: validation happens before the library is asked to compute).

The refusals are generated from one literal table per gateway, ARGS below, written from the reference's argument lists
(the header comment of each gateway) -- not from the gateways' code.  Every generated case asserts the exact
identifier, that the message names the gateway and the argument, and that the refused call left no mxArray behind."""
import ctypes
import os
import numpy as np
import pytest

from fsgm_amd import synth, _lib
from tests import mexharness as mh

GATEWAYS = ["calc_cost_sgm", "calc_cost_sgm_linear", "calc_pyd_cost_sgm", "calc_pyd_cost_sgm_ng", "calc_cost_sgm_ng",
            "fsgm_pyramidal_sgm", "fsgm_pyramidal_sgm_ng"]


@pytest.mark.parametrize("name", GATEWAYS)
def test_gateway_exports_mexfunction(name):
    mh.stub()
    lib = ctypes.CDLL(os.path.join(mh.MEXDIR, f"{name}.mexstub.so"))
    assert hasattr(lib, "mexFunction")


def _epi_args(W=32, H=24, D=16):
    I1, I2 = synth.image_pair(W, H, D)
    pd0, nd, off = synth.epi_maps(W, H)
    return [I1, I2, D, 0.3, pd0, nd, off, 6, 64]


def test_wrong_argument_count_and_classes():
    a = _epi_args()
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *a[:8])
    assert e.value.ident == "fsgm:nrhs"
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 5, *a)
    assert e.value.ident == "fsgm:nlhs"
    b = list(a); b[0] = a[0].astype(np.float64)
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *b)
    assert e.value.ident == "fsgm:class"
    b = list(a); b[1] = a[1][:, :-1]
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *b)
    assert e.value.ident == "fsgm:size"
    b = list(a); b[4] = a[4][0]
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *b)
    assert e.value.ident == "fsgm:size"
    b = list(a); b[2] = 0
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *b)
    assert e.value.ident == "fsgm:range"


def test_pyd_gateway_validation():
    I1, I2 = synth.image_pair(20, 16, 16)
    mv = synth.hint_map(20, 16)
    with pytest.raises(mh.MexError) as e:                  # hint map smaller than the image
        mh.call("calc_pyd_cost_sgm", 3, I1, I2, mv[:, :10, :], 5, 5, 2, 0, 6, 32, 1, 2, 0)
    assert e.value.ident == "fsgm:size"
    with pytest.raises(mh.MexError) as e:                  # fractional window half size
        mh.call("calc_pyd_cost_sgm", 3, I1, I2, mv, 2.5, 5, 2, 0, 6, 32, 1, 2, 0)
    assert e.value.ident == "fsgm:range"
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_pyd_cost_sgm_ng", 2, I1, I2, mv, 1, 2, 0, 6)
    assert e.value.ident == "fsgm:nrhs"


def test_pyramid_gateway_validation():
    I0, I1 = synth.image_pair(20, 16, 8)
    with pytest.raises(mh.MexError) as e:
        mh.call("fsgm_pyramidal_sgm", 2, I0)
    assert e.value.ident == "fsgm:nrhs"
    with pytest.raises(mh.MexError) as e:                  # two planes: neither gray nor RGB
        mh.call("fsgm_pyramidal_sgm", 2, np.stack([I0, I0]), np.stack([I1, I1]), 3)
    assert e.value.ident == "fsgm:size"
    with pytest.raises(mh.MexError) as e:
        mh.call("fsgm_pyramidal_sgm", 2, I0, I1[:, :-1], 3)
    assert e.value.ident == "fsgm:size"
    with pytest.raises(mh.MexError) as e:
        mh.call("fsgm_pyramidal_sgm", 2, I0, I1, 0)
    assert e.value.ident == "fsgm:range"
    with pytest.raises(mh.MexError) as e:                  # more outputs than mv, minC and one flow per level
        mh.call("fsgm_pyramidal_sgm", 6, I0, I1, 3)
    assert e.value.ident == "fsgm:nlhs"


def test_no_gpu_is_a_mex_error_not_a_fallback():
    if _lib.load().fsgm_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(mh.MexError) as e:
        mh.call("calc_cost_sgm", 2, *_epi_args())
    assert e.value.ident == "fsgm:hip" and "no HIP device" in str(e.value)
    assert e.value.leaked == 0                             # the outputs the gateway had created for the refused call are gone


# ------------------------------------------------------------------------------------------------ the harness itself
def test_stub_scalars_convert_like_matlab():
    """mxGetScalar of a 1x1 of each class is the value as a double"""
    assert mh.scalar_of(0.3) == 0.3
    assert mh.scalar_of(np.float32(0.3)) == float(np.float32(0.3)) != 0.3
    assert mh.scalar_of(np.int32(-7)) == -7.0 and mh.scalar_of(np.int32(2 ** 31 - 1)) == 2.0 ** 31 - 1
    assert mh.scalar_of(np.uint32(2 ** 32 - 1)) == 2.0 ** 32 - 1
    assert mh.scalar_of(np.bool_(True)) == 1.0 and mh.scalar_of(np.bool_(False)) == 0.0
    assert mh.scalar_of(np.int8(-3)) == -3.0 and mh.scalar_of(np.uint16(65535)) == 65535.0 and mh.scalar_of(np.int16(-300)) == -300.0
    assert mh.scalar_of(np.int64(-2 ** 40)) == -2.0 ** 40 and mh.scalar_of(np.uint8(200)) == 200.0
    assert mh.scalar_of(np.array([4.5, 7.0])) == 4.5                  # the first element of an array


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.uint8, np.uint32, np.int32, np.bool_])
def test_stub_arrays_round_trip_and_are_counted(dt):
    s = mh.stub()
    before = mh.live_arrays()
    a = (np.arange(2 * 3 * 5).reshape(2, 3, 5) % 7).astype(dt)
    made = [mh.to_mx(a), mh.to_mx(mh.Arr(a, (5, 3, 2, 1))), mh.to_mx(mh.Arr(a[:1], (5, 3, 1))), mh.to_mx(np.zeros((4, 0), dt)),
            mh.to_mx(np.zeros((0, 4), dt)), mh.to_mx(dt(1)), mh.to_mx(1.5)]
    assert mh.live_arrays() == before + len(made)
    assert [mh.dims_of(m) for m in made] == [(5, 3, 2), (5, 3, 2, 1), (5, 3, 1), (0, 4), (4, 0), (1, 1), (1, 1)]
    back = mh.from_mx(made[0])
    assert back.dtype == np.dtype(dt) and np.array_equal(back, a)
    assert np.array_equal(mh.from_mx(made[1])[0], a) and mh.from_mx(made[3]).shape == (4, 0)
    assert mh.from_mx(made[5]).dtype == np.dtype(dt) and mh.from_mx(made[6]).dtype == np.float64
    for m in made:
        s.mxDestroyArray(m)
    assert mh.live_arrays() == before


# ------------------------------------------------------------------------------------------------ the argument tables
# One row per argument, in the order of the reference's call: (name, kind, ...).
#   u8      uint8 image, W x H, 2-D                       u8p     uint8 image, W x H or W x H x 3 (the pyramid drivers)
#   f64 n   double array of n elements (n in W, H)        hint    preMv: double, mvW x (2 mvH), mvW >= W, mvH >= H
#   hint1   preMv: double, mvW x N with N >= 2 (the neighbour-guided matcher clamps into it, ng_sgm.m hands it W x H)
#   f64any  a double array of any size (read, not used)
#   int     scalar, C truncation to int                   whole lo  scalar, a whole number >= lo
#   real    scalar, any double                            bool    scalar, != 0
# "bad" lists further values of a scalar that are out of range for this argument.
W, H = 20, 12
ARGS = {
    "calc_cost_sgm": dict(nrhs=9, nlhs=4, rows=[
        ("I1", "u8"), ("I2", "u8"), ("dMax", "int", dict(bad=(0, -3))), ("vMax", "real"), ("pixelPosD0", "f64", 2 * W * H),
        ("normlizeDirection", "f64", 2 * W * H), ("offsetFromPosD0", "f64", W * H), ("P1", "int"), ("P2", "int")]),
    "calc_cost_sgm_linear": dict(nrhs=9, nlhs=4, rows=[
        ("I1", "u8"), ("I2", "u8"), ("dMax", "int", dict(bad=(0, -3))), ("vMax", "real"), ("pixelPosD0", "f64", 2 * W * H),
        ("normlizeDirection", "f64", 2 * W * H), ("offsetFromPosD0", "f64", W * H), ("P1", "int"), ("P2", "int")]),
    "calc_pyd_cost_sgm": dict(nrhs=12, nlhs=3, rows=[
        ("I1", "u8"), ("I2", "u8"), ("preMv", "hint"), ("halfSearchWinSizeX", "whole", 0), ("halfSearchWinSizeY", "whole", 0),
        ("aggHalfWinSize", "whole", 0), ("subPixelRefine", "int"), ("P1", "int"), ("P2", "int"), ("enableDiagnalPath", "bool"),
        ("totalPass", "int"), ("adpativeP2", "bool")]),
    "calc_pyd_cost_sgm_ng": dict(nrhs=8, nlhs=2, rows=[
        ("I1", "u8"), ("I2", "u8"), ("preMv", "hint1"), ("halfSearchWinSize", "int", dict(bad=(-1, 4, 23170, 1e6))),
        ("aggSize", "int", dict(bad=(-1,))), ("subPixelRefine", "int"), ("P1", "int"), ("P2", "int")]),
    "calc_cost_sgm_ng": dict(nrhs=8, nlhs=2, rows=[
        ("I1", "u8"), ("I2", "u8"), ("preMv", "f64any"), ("halfSearchWinSize", "real"), ("aggSize", "real"),
        ("subPixelRefine", "int"), ("P1", "int"), ("P2", "int")]),
    "fsgm_pyramidal_sgm": dict(nrhs=3, nlhs="2+numPyd", rows=[("I0", "u8p"), ("I1", "u8p"), ("numPyd", "whole", 1, dict(bad=(0, 17)))]),
    "fsgm_pyramidal_sgm_ng": dict(nrhs=3, nlhs="2+numPyd", rows=[("I0", "u8p"), ("I1", "u8p"), ("numPyd", "whole", 1, dict(bad=(0, 17)))]),
}
NUMPYD = 3
_good = {}


def good_args(gw):
    """a call the gateway's checks accept, W x H = 20 x 12"""
    if gw not in _good:
        I1, I2 = synth.image_pair(W, H, 8, seed=2)
        if gw in ("calc_cost_sgm", "calc_cost_sgm_linear"):
            pd0, nd, off = synth.epi_maps(W, H)
            _good[gw] = [I1, I2, 16, 0.3, pd0, nd, off, 6, 64]
        elif gw == "calc_pyd_cost_sgm":
            _good[gw] = [I1, I2, synth.hint_map(W, H), 2, 1, 2, 1, 6, 32, 1, 2, 0]
        elif gw in ("calc_pyd_cost_sgm_ng", "calc_cost_sgm_ng"):
            _good[gw] = [I1, I2, synth.hint_map(W, H), 1, 2, 0, 6, 32]
        else:
            _good[gw] = [I1, I2, NUMPYD]
    return list(_good[gw])


def _empty():
    return mh.Arr(np.zeros(0), (0, 0))


def _image_cases(a, planes):
    """(label, value, identifier) for a uint8 image argument a: (H, W), or (3, H, W) where planes are allowed"""
    yield "double", a.astype(np.float64), "fsgm:class"
    yield "uint32", a.astype(np.uint32), "fsgm:class"
    if planes:
        yield "4d", mh.Arr(np.stack([a, a]), (W, H, 1, 2)), "fsgm:class"
        yield "two_planes", np.stack([a, a]), "fsgm:size"
    else:
        yield "3d", np.stack([a, a]), "fsgm:class"
    yield "transposed", np.ascontiguousarray(a.T), "fsgm:size"
    yield "column_short", np.ascontiguousarray(a[:, :-1]), "fsgm:size"
    yield "0xH", np.zeros((H, 0), np.uint8), "fsgm:size"
    yield "Wx0", np.zeros((0, W), np.uint8), "fsgm:size"


def _row_cases(row, good):
    name, kind = row[0], row[1]
    extra = row[-1] if isinstance(row[-1], dict) else {}
    if kind in ("u8", "u8p"):
        yield from _image_cases(good, kind == "u8p")
        return
    if kind in ("f64", "hint", "hint1", "f64any"):
        yield "uint8", np.zeros(np.shape(good), np.uint8), "fsgm:class"
    if kind == "f64":
        n = row[2]
        assert np.size(good) == n                                     # the table against the good call
        yield "short", np.zeros(n - 1), "fsgm:size"
        yield "over", np.zeros(n + 1), "fsgm:size"
    if kind == "hint":
        yield "odd_N", mh.Arr(np.zeros(W * (2 * H + 1)), (W, 2 * H + 1)), "fsgm:size"
        yield "mvW_short", np.zeros((2, H, W - 1)), "fsgm:size"
        yield "mvH_short", np.zeros((2, H - 1, W)), "fsgm:size"
        yield "empty", _empty(), "fsgm:size"
    if kind == "hint1":
        yield "N_1", mh.Arr(np.zeros(W), (W, 1)), "fsgm:size"
        yield "empty", _empty(), "fsgm:size"
    if kind in ("int", "whole", "real", "bool"):
        yield "1x2", mh.Arr(np.array([float(good), float(good)]), (1, 2)), "fsgm:size"
        yield "empty", _empty(), "fsgm:size"
    if kind == "int":
        for label, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("2^31", 2.0 ** 31), ("-2^31-1", -2.0 ** 31 - 1)):
            yield label, v, "fsgm:range"
    if kind == "whole":
        for label, v in (("2.5", 2.5), ("-1", -1.0), ("1e6+1", 1e6 + 1), ("nan", np.nan)):
            yield label, v, "fsgm:range"
    for v in extra.get("bad", ()):
        yield f"bad_{v:g}", v, "fsgm:range"


def _cases():
    for gw, t in ARGS.items():
        rows, nrhs = t["rows"], t["nrhs"]
        assert len(rows) == nrhs
        max_nlhs = 2 + NUMPYD if t["nlhs"] == "2+numPyd" else t["nlhs"]
        pyramid = t["nlhs"] == "2+numPyd"
        # argument and output counts (the pyramid drivers take 2 or 3 inputs: 1 and 4 are refused)
        yield gw, "nrhs_short", ("drop" if not pyramid else "drop2"), 1, "fsgm:nrhs", "inputs"
        yield gw, "nrhs_over", "extra", 1, "fsgm:nrhs", "inputs"
        yield gw, "nlhs_over", None, max_nlhs + 1, "fsgm:nlhs", "outputs"
        for k, row in enumerate(rows):
            yield gw, row[0], k, 1, None, None
    # the window of calc_pyd_cost_sgm: half sizes whose candidate count would not fit an int, and windows the library refuses
    for label, hx, hy in (("1e6", 1e6, 1e6), ("32_0", 32, 0), ("0_32", 0, 32), ("31_31", 31, 31), ("23170", 23170, 23170), ("16_16", 16, 16)):
        yield "calc_pyd_cost_sgm", f"window_{label}", ("window", hx, hy), 3, "fsgm:range", "halfSearchWinSize"


def _expand():
    out = []
    for gw, what, k, nlhs, ident, token in _cases():
        if ident is not None:
            out.append(pytest.param(gw, k, None, nlhs, ident, token, id=f"{gw}-{what}"))
            continue
        good = _placeholder_good(gw, k)
        for label, _, cid in _row_cases(ARGS[gw]["rows"][k], good):
            if gw == "calc_cost_sgm" and k == 0 and label == "3d":
                continue                                              # a 3-D I1 is calc_cost_sgm's batch form: below
            out.append(pytest.param(gw, k, label, nlhs, cid, ARGS[gw]["rows"][k][0], id=f"{gw}-{what}-{label}"))
    return out


def _placeholder_good(gw, k):
    return good_args(gw)[k]


def _refused(gw, nlhs, args, ident, token):
    with pytest.raises(mh.MexError) as e:
        mh.call_full(gw, nlhs, *args)
    assert e.value.ident == ident, str(e.value)
    assert e.value.msg.startswith(gw + ":") and token in e.value.msg, e.value.msg
    assert e.value.leaked == 0, f"{e.value.leaked} mxArrays left behind by the refused call"
    assert mh.live_arrays() == e.value.live_before


@pytest.mark.parametrize("gw,k,label,nlhs,ident,token", _expand())
def test_refusals_from_the_argument_tables(gw, k, label, nlhs, ident, token):
    args = good_args(gw)
    if label is None:
        if k == "drop":
            args = args[:-1]
        elif k == "drop2":
            args = args[:1]
        elif k == "extra":
            args = args + [1]
        elif isinstance(k, tuple):
            args[3], args[4] = k[1], k[2]
    else:
        value = {lab: v for lab, v, _ in _row_cases(ARGS[gw]["rows"][k], args[k])}[label]
        args[k] = value
    _refused(gw, nlhs, args, ident, token)


# ------------------------------------------------------------------------------------------------ calc_cost_sgm's batch form
N = 3


def _batch_args(n=N):
    a = good_args("calc_cost_sgm")
    rep = lambda x: np.ascontiguousarray(np.stack([x] * n))  # noqa: E731
    return [rep(a[0]), rep(a[1]), a[2], a[3], rep(a[4]), rep(a[5]), rep(a[6]), a[7], a[8]]


BATCH_CASES = [                                            # (label, argument index, value from the good batch, identifier, token)
    ("I1_double", 0, lambda a: a[0].astype(np.float64), "fsgm:class", "I1"),
    ("I2_uint32", 1, lambda a: a[1].astype(np.uint32), "fsgm:class", "I2"),
    ("I2_2d", 1, lambda a: a[1][0], "fsgm:size", "I2"),
    ("I2_other_n", 1, lambda a: a[1][:N - 1], "fsgm:size", "I2"),
    ("I2_transposed", 1, lambda a: np.ascontiguousarray(a[1].transpose(0, 2, 1)), "fsgm:size", "I2"),
    ("pixelPosD0_n-1", 4, lambda a: a[4][:N - 1], "fsgm:size", "pixelPosD0"),
    ("normlizeDirection_n-1", 5, lambda a: a[5][:N - 1], "fsgm:size", "normlizeDirection"),
    ("offsetFromPosD0_n-1", 6, lambda a: a[6][:N - 1], "fsgm:size", "offsetFromPosD0"),
    ("pixelPosD0_uint8", 4, lambda a: a[4].astype(np.uint8), "fsgm:class", "pixelPosD0"),
    ("n_0", 0, lambda a: np.zeros((0, H, W), np.uint8), "fsgm:size", "I1"),
    ("dMax_0", 2, lambda a: 0, "fsgm:range", "dMax"),
    ("dMax_nan", 2, lambda a: np.nan, "fsgm:range", "dMax"),
    ("P2_2^31", 8, lambda a: 2.0 ** 31, "fsgm:range", "P2"),
    ("vMax_1x2", 3, lambda a: mh.Arr(np.array([0.3, 0.3]), (1, 2)), "fsgm:size", "vMax"),
]


@pytest.mark.parametrize("case", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_form_refusals(case):
    _, k, make, ident, token = case
    a = _batch_args()
    a[k] = make(a)
    _refused("calc_cost_sgm", 4, a, ident, token)


@pytest.mark.parametrize("env,ident,token", [({"FSGM_DEVICES": "0,x"}, "fsgm:invalid", "FSGM_DEVICES"),
                                             ({"FSGM_EPI_ADAPTIVE_P2": "1", "FSGM_DEVICES": "0,1"}, "fsgm:unsupported", "FSGM_EPI_ADAPTIVE_P2")],
                         ids=["device_list_0,x", "adaptive_p2_with_two_devices"])
def test_batch_form_refuses_its_environment_before_it_creates_anything(monkeypatch, env, ident, token):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _refused("calc_cost_sgm", 4, _batch_args(), ident, token)
