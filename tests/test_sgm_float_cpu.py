"""CPU-side tests of the float cost-volume entries (include/fsgm.h, "Float cost volumes"): the numpy restatement of the
quantising rule on hand-worked values, every refusal of the six C entries that answers before a device is touched, the Python
wrappers' TypeErrors, the two ops of the fsgm_float namespace under FakeTensorMode, and that the u8 wrappers still refuse floats."""
import ctypes as C

import numpy as np
import pytest

try:                                     # torch first where it is installed: the library must bind to its HIP runtime
    import torch  # noqa: F401
except ImportError:
    torch = None

import fsgm_amd  # noqa: E402
from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.sgm import CostFormat, _bind as _bind_sgm, cost_format  # noqa: E402
from fsgm_amd.sgm2d import _bind as _bind_sgm2d  # noqa: E402
from tests import cost_quant_restatement as Q  # noqa: E402

FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
FAKE = C.c_void_p(0x1000)                # never dereferenced: every call it goes into fails its argument checks first
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _bind_sgm2d(_bind_sgm(_lib.load()))


def _err(lib):
    return lib.fsgm_last_error().decode()


def _q(values, scale=1.0, offset=0.0, bound=255):
    q, flagged = Q.quantise(np.array(values, f32), scale, offset, bound)
    return q.tolist(), flagged.tolist()


# ---- 1. the restatement on hand-worked values ----
def test_ties_go_to_even():
    # k + 0.5 for even k rounds down to k, for odd k up to k + 1
    assert _q([0.5, 1.5, 2.5, 3.5, 100.5, 101.5, 253.5]) == ([0, 2, 2, 4, 100, 102, 254], [False] * 7)


def test_the_upper_bound_and_its_neighbours():
    for B in (255, 24):                                          # odd and even: B + 0.5 ties up to B + 1, and down to B
        above = np.nextafter(f32(B + 0.5), f32(np.inf))
        below = np.nextafter(f32(B + 0.5), f32(-np.inf))
        q, fl = _q([below, B + 0.5, above, B, B + 1], bound=B)
        tie_flagged = B % 2 == 1                                 # rint(255.5) = 256 > 255; rint(24.5) = 24
        assert q == [B] * 5 and fl == [False, tie_flagged, True, False, True]


def test_the_lower_bound_zeros_nan_and_infinities():
    q, fl = _q([-0.5, -0.0, 0.0, -0.4, -0.6, -1.0, np.nan, np.inf, -np.inf], bound=200)
    #            rint(-0.5) = -0.0: not below 0;          -0.6 -> -1 < 0;  NaN and +inf -> B;  -inf -> 0
    assert q == [0, 0, 0, 0, 0, 0, 200, 200, 0]
    assert fl == [False, False, False, False, True, True, True, True, True]


def test_a_scale_whose_product_rounds():
    """scale 0.1 is 0x3DCCCCCD, a little above a tenth: 25 * scale = 2.500000037..., which fp32 rounds to 2.5 exactly (its
    neighbours are 2.4e-7 away), so rint gives the tie's 2 -- a double product would be above 2.5 and give 3."""
    assert float(f32(25) * f32(0.1)) == 2.5
    assert int(np.rint(25 * float(f32(0.1)))) == 3               # what a rule in double would have answered
    assert _q([25.0], scale=0.1) == ([2], [False])
    # the multiply and the add round separately: 8193 * 8191 = 2^26 - 1 needs 26 bits and rounds to 2^26, and the offset
    # -(2^26 - 4) = -4 * 16777215 is an fp32 number -- the rule gives 2^26 - (2^26 - 4) = 4, a fused multiply-add would give 3
    x, s, o = f32(8193), f32(8191), -(2.0 ** 26 - 4)
    assert float(x * s) == 2.0 ** 26 and float(f32(o)) == o
    assert _q([x], scale=s, offset=o) == ([4], [False])
    # a negative scale turns a similarity into a cost
    assert _q([1.0, 0.5, 0.0, -0.25], scale=-100.0, offset=100.0, bound=120) == ([0, 50, 100, 120], [False, False, False, True])


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_identity_on_bytes(dtype):
    """a uint8 volume cast to each float type (0..255 are exact in all three) with scale 1, offset 0 quantises to itself"""
    v = np.arange(256, dtype=np.uint8)
    if dtype == "bfloat16":
        torch_ = pytest.importorskip("torch")
        x = torch_.from_numpy(v).to(torch_.bfloat16).to(torch_.float32).numpy()
    else:
        x = v.astype(dtype).astype(f32)
    q, fl = Q.quantise(x, 1.0, 0.0, 255)
    assert np.array_equal(q, v) and not fl.any()


# ---- 2. refusals without a device ----
def _fmt(dtype=0, scale=1.0, offset=0.0):
    f = CostFormat()
    f.dtype, f.scale, f.offset = dtype, scale, offset
    return f


def _sgm_host(lib, fmt, **kw):
    a = dict(n=1, Cp=FAKE, W=32, H=24, D=16, P1=7, P2=100, prm=None, guide=None, bestD=FAKE, minC=FAKE, minC2=None, S=None, exact=0)
    a.update(kw)
    return lib.fsgm_sgm_float_batch_host(a["n"], a["Cp"], fmt, a["W"], a["H"], a["D"], a["P1"], a["P2"], a["prm"], a["guide"], a["bestD"],
                                         a["minC"], a["minC2"], a["S"], a["exact"])


def _sgm_dptr(lib, fmt, **kw):
    a = dict(n=1, Cp=FAKE, W=32, H=24, D=16, P1=7, P2=100, prm=None, guide=None, bestD=FAKE, minC=FAKE, minC2=None, S=None, exact=0)
    a.update(kw)
    return lib.fsgm_sgm_float_dptr(a["n"], a["Cp"], fmt, a["W"], a["H"], a["D"], a["P1"], a["P2"], a["prm"], a["guide"], a["bestD"],
                                   a["minC"], a["minC2"], a["S"], a["exact"], None, None)


def _sgm2d_args(kw):
    a = dict(n=1, Cp=FAKE, W=32, H=24, rX=1, rY=2, P1=6, P2=32, prm=None, preMv=None, mvW=0, mvH=0, guide=None, bestD=FAKE, minC=FAKE,
             minC2=None, mvSub=FAKE, flow=None, S=None, exact=0)
    a.update(kw)
    return a


def _sgm2d_host(lib, fmt, **kw):
    a = _sgm2d_args(kw)
    return lib.fsgm_sgm2d_float_batch_host(a["n"], a["Cp"], fmt, a["W"], a["H"], a["rX"], a["rY"], a["P1"], a["P2"], a["prm"], a["preMv"],
                                           a["mvW"], a["mvH"], a["guide"], a["bestD"], a["minC"], a["minC2"], a["mvSub"], a["flow"], a["S"],
                                           a["exact"])


def _sgm2d_dptr(lib, fmt, **kw):
    a = _sgm2d_args(kw)
    return lib.fsgm_sgm2d_float_dptr(a["n"], a["Cp"], fmt, a["W"], a["H"], a["rX"], a["rY"], a["P1"], a["P2"], a["prm"], a["preMv"],
                                     a["mvW"], a["mvH"], a["guide"], a["bestD"], a["minC"], a["minC2"], a["mvSub"], a["flow"], a["S"],
                                     a["exact"], None, None)


def _epi_ingest(lib, fmt, **kw):
    a = dict(plan=FAKE, Cp=FAKE)
    a.update(kw)
    return lib.fsgm_epi_plan_ingest_float_dptr(a["plan"], 1, a["Cp"], fmt, 1, 255, None, None)


def _pyd_ingest(lib, fmt, **kw):
    a = dict(plan=FAKE, Cp=FAKE)
    a.update(kw)
    return lib.fsgm_pyd_plan_ingest_float_dptr(a["plan"], 1, a["Cp"], fmt, 1, 255, None, None)


ENTRIES = {"sgm_host": _sgm_host, "sgm_dptr": _sgm_dptr, "sgm2d_host": _sgm2d_host, "sgm2d_dptr": _sgm2d_dptr, "epi_ingest": _epi_ingest,
           "pyd_ingest": _pyd_ingest}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_bad_cost_format_is_refused_by_every_entry(lib, entry):
    call = ENTRIES[entry]
    assert call(lib, None) == FSGM_ERR_INVALID and "null fmt" in _err(lib)
    for dtype in (-1, 3, 100):
        assert call(lib, C.byref(_fmt(dtype=dtype))) == FSGM_ERR_INVALID and "dtype" in _err(lib)
    for scale in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        assert call(lib, C.byref(_fmt(scale=scale))) == FSGM_ERR_INVALID and "scale" in _err(lib)
    for offset in (float("inf"), float("-inf"), float("nan")):
        assert call(lib, C.byref(_fmt(offset=offset))) == FSGM_ERR_INVALID and "offset" in _err(lib)
    for word in range(5):
        f = _fmt()
        f.reserved[word] = 1
        assert call(lib, C.byref(f)) == FSGM_ERR_INVALID and "reserved words of fsgm_cost_format" in _err(lib)
    assert call(lib, C.byref(_fmt()), Cp=None) == FSGM_ERR_INVALID and "null" in _err(lib)


def test_the_default_format(lib):
    f = lib.fsgm_cost_format_default()
    assert (f.dtype, f.scale, f.offset, list(f.reserved)) == (0, 1.0, 0.0, [0] * 5)
    assert C.sizeof(CostFormat) == 32


@pytest.mark.parametrize("call", [_sgm_host, _sgm_dptr], ids=["host", "dptr"])
def test_sgm_float_refuses_what_the_u8_forms_refuse(lib, call):
    fmt = C.byref(_fmt(dtype=1, scale=-3.0, offset=2.0))
    for kw, word in (({"n": 0}, "n_frames"), ({"W": 0}, "width"), ({"H": -1}, "width"), ({"D": 0}, "dMax"), ({"D": 1025}, "dMax"),
                     ({"bestD": None}, "null"), ({"minC": None}, "null"), ({"exact": 2}, "exact"), ({"exact": -1}, "exact"),
                     ({"exact": 1, "P1": 256}, "0..255"), ({"exact": 1, "P2": -1}, "0..255")):
        assert call(lib, fmt, **kw) == FSGM_ERR_INVALID and word in _err(lib), (kw, _err(lib))
    for field, bad, word in (("paths", 5, "paths"), ("subpixel", 2, "subpixel"), ("layout", 2, "layout"), ("cost_bound", 0, "cost_bound"),
                             ("cost_bound", 256, "cost_bound"), ("agg_mode", 7, "agg_mode"), ("adaptive_p2", 2, "adaptive_p2")):
        p = lib.fsgm_sgm_params_default()
        setattr(p, field, bad)
        assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and word in _err(lib), (field, _err(lib))
    p = lib.fsgm_sgm_params_default()
    p.reserved[2] = 1
    assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and "reserved words of fsgm_sgm_params" in _err(lib)
    p = lib.fsgm_sgm_params_default()
    p.adaptive_p2 = 1
    assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and "guide" in _err(lib)
    # FSGM_ERR_UNSUPPORTED: exact with minC2; agg_mode 2..6 with exact, minC2 or adaptive P2; too large a volume or batch
    assert call(lib, fmt, exact=1, minC2=FAKE) == FSGM_ERR_UNSUPPORTED and "runner-up" in _err(lib)
    for mode in range(2, 7):
        p = lib.fsgm_sgm_params_default()
        p.agg_mode = mode
        assert call(lib, fmt, prm=C.byref(p), exact=1) == FSGM_ERR_UNSUPPORTED and "line kernels" in _err(lib)
        assert call(lib, fmt, prm=C.byref(p), minC2=FAKE) == FSGM_ERR_UNSUPPORTED and "line kernels" in _err(lib)
        p.adaptive_p2 = 1
        assert call(lib, fmt, prm=C.byref(p), guide=FAKE) == FSGM_ERR_UNSUPPORTED and "line kernels" in _err(lib)
    assert call(lib, fmt, W=4096, H=4096, D=128) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)
    assert call(lib, fmt, n=65536) == FSGM_ERR_UNSUPPORTED and "65535" in _err(lib)


@pytest.mark.parametrize("call", [_sgm2d_host, _sgm2d_dptr], ids=["host", "dptr"])
def test_sgm2d_float_refuses_what_the_u8_forms_refuse(lib, call):
    fmt = C.byref(_fmt(dtype=2, scale=0.5))
    for kw, word in (({"n": 0}, "n_frames"), ({"W": 0}, "width"), ({"rX": -1}, "halfX"), ({"bestD": None}, "null"), ({"minC": None}, "null"),
                     ({"mvSub": None}, "null"), ({"exact": 2}, "exact"), ({"exact": 1, "P1": 256}, "0..255"), ({"exact": 1, "P2": -1}, "0..255"),
                     ({"preMv": FAKE, "mvW": 31, "mvH": 24}, "preMv")):
        assert call(lib, fmt, **kw) == FSGM_ERR_INVALID and word in _err(lib), (kw, _err(lib))
    for field, bad, word in (("layout", 3, "layout"), ("cost_bound", 0, "cost_bound"), ("cost_bound", 256, "cost_bound"),
                             ("totalPass", 3, "totalPass"), ("diagonal", 2, "diagonal"), ("adaptive_p2", -1, "adaptive_p2"),
                             ("subpixel", 2, "subpixel")):
        p = lib.fsgm_sgm2d_params_default()
        setattr(p, field, bad)
        assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and word in _err(lib), (field, _err(lib))
    p = lib.fsgm_sgm2d_params_default()
    p.reserved[4] = 7
    assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and "reserved words of fsgm_sgm2d_params" in _err(lib)
    p = lib.fsgm_sgm2d_params_default()
    p.adaptive_p2 = 1
    assert call(lib, fmt, prm=C.byref(p)) == FSGM_ERR_INVALID and "guide" in _err(lib)
    assert call(lib, fmt, rX=32, rY=0) == FSGM_ERR_UNSUPPORTED                       # a side of 65
    assert call(lib, fmt, rX=16, rY=16) == FSGM_ERR_UNSUPPORTED                      # 1089 candidates
    assert call(lib, fmt, W=8192, H=8192, rX=4, rY=4) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)
    assert call(lib, fmt, n=65536) == FSGM_ERR_UNSUPPORTED and "65535" in _err(lib)


@pytest.mark.parametrize("call", [_epi_ingest, _pyd_ingest], ids=["epi", "pyd"])
def test_plan_ingests_refuse_a_null_plan(lib, call):
    assert call(lib, C.byref(_fmt()), plan=None) == FSGM_ERR_INVALID and "null argument" in _err(lib)


# ---- 3. the Python wrappers ----
def test_numpy_wrappers_type_errors():
    for bad in (np.zeros((5, 7, 16), np.uint8), np.zeros((5, 7, 16), np.float64), np.zeros((5, 7, 16), np.int32)):
        with pytest.raises(TypeError, match="float32 or float16"):
            fsgm_amd.sgm_batch_float(bad, 1.0)
    for bad in (np.zeros((9, 5, 7), np.uint8), np.zeros((9, 5, 7), np.float64)):
        with pytest.raises(TypeError, match="float32 or float16"):
            fsgm_amd.sgm2d_batch_float(bad, 1, 1, 1.0)
    Cv = np.zeros((5, 7, 16), np.float32)
    with pytest.raises(TypeError, match="guide"):
        fsgm_amd.sgm_batch_float(Cv, 1.0, guide=np.zeros((5, 7), np.float32), adaptive_p2=1)
    with pytest.raises(TypeError, match=r"\(H, W, D\)"):
        fsgm_amd.sgm_batch_float(np.zeros((5, 7), np.float32), 1.0)
    with pytest.raises(ValueError, match="runner"):
        fsgm_amd.sgm_batch_float(Cv, 1.0, arith="exact", runner_up=True)
    with pytest.raises(ValueError, match="arith"):
        fsgm_amd.sgm_batch_float(Cv, 1.0, arith="saturate")
    with pytest.raises(ValueError, match="layout"):
        fsgm_amd.sgm_batch_float(Cv, 1.0, layout="whd")
    with pytest.raises(ValueError, match="candidates"):
        fsgm_amd.sgm2d_batch_float(np.zeros((8, 5, 7), np.float16), 1, 1, 1.0)
    with pytest.raises(TypeError, match="hints"):
        fsgm_amd.sgm2d_batch_float(np.zeros((9, 5, 7), np.float16), 1, 1, 1.0, hints=np.zeros((2, 5, 7), np.float32))
    # the library's own refusals arrive as FsgmError: a zero scale, an agg_mode the runner-up cost cannot take
    with pytest.raises(_lib.FsgmError) as e:
        fsgm_amd.sgm_batch_float(Cv, 0.0)
    assert e.value.status == FSGM_ERR_INVALID
    with pytest.raises(_lib.FsgmError) as e:
        fsgm_amd.sgm2d_batch_float(np.zeros((9, 5, 7), np.float32), 1, 1, float("nan"))
    assert e.value.status == FSGM_ERR_INVALID
    with pytest.raises(_lib.FsgmError) as e:
        fsgm_amd.sgm_batch_float(Cv, 1.0, runner_up=True, agg_mode=4)
    assert e.value.status == FSGM_ERR_UNSUPPORTED


def test_cost_format_helper():
    f = cost_format(np.dtype("float16"), 0.1, 3)
    assert (f.dtype, f.scale, f.offset) == (1, float(f32(0.1)), 3.0)
    assert cost_format("bfloat16", 2).dtype == 2 and cost_format(np.float32, 2).dtype == 0
    for bad in (np.uint8, np.float64, "int8"):
        with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
            cost_format(bad, 1.0)


def test_the_u8_numpy_wrappers_still_refuse_floats():
    for dt in (np.float32, np.float16):
        with pytest.raises(TypeError, match="uint8"):
            fsgm_amd.sgm_batch(np.zeros((5, 7, 16), dt))
        with pytest.raises(TypeError, match="uint8"):
            fsgm_amd.sgm2d_batch(np.zeros((9, 5, 7), dt), 1, 1)


def test_new_symbols_are_exported(lib):
    for name in ("fsgm_cost_format_default", "fsgm_epi_plan_ingest_float_dptr", "fsgm_pyd_plan_ingest_float_dptr", "fsgm_sgm_float_dptr",
                 "fsgm_sgm2d_float_dptr", "fsgm_sgm_float_batch_host", "fsgm_sgm2d_float_batch_host"):
        assert hasattr(lib, name), name
    assert callable(fsgm_amd.sgm_batch_float) and callable(fsgm_amd.sgm2d_batch_float)
    with open(_lib.__file__.replace("fsgm_amd/_lib.py", "include/fsgm.h")) as f:
        header = f.read()
    for name in ("FSGM_COST_F32 0", "FSGM_COST_F16 1", "FSGM_COST_BF16 2", "fsgm_cost_format;"):
        assert name in header, name


# ---- 4. the torch ops ----
def _torch_ops():
    pytest.importorskip("torch")
    from fsgm_amd import torch_ops
    return torch_ops


def test_ops_live_in_their_own_namespace():
    _torch_ops()
    sgm_schema = str(torch.ops.fsgm_float.sgm.default._schema)
    assert sgm_schema == ("fsgm_float::sgm(Tensor C_, Tensor guide, float scale, float offset, SymInt P1, SymInt P2, SymInt paths, SymInt layout, "
                          "SymInt cost_bound, SymInt agg_mode, SymInt adaptive_p2, SymInt subpixel, SymInt return_sum, bool runner_up, "
                          "bool exact) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
    sgm2d_schema = str(torch.ops.fsgm_float.sgm2d.default._schema)
    assert sgm2d_schema == ("fsgm_float::sgm2d(Tensor C_, Tensor hints, Tensor guide, float scale, float offset, SymInt half_x, SymInt half_y, "
                            "SymInt P1, SymInt P2, SymInt layout, SymInt cost_bound, SymInt diagonal, SymInt total_pass, SymInt adaptive_p2, "
                            "SymInt subpixel, SymInt return_flow, SymInt return_sum, bool runner_up, bool exact) -> "
                            "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    # the u8 families' schemas with scale and offset behind the tensors and the two flags at the end
    u8 = str(torch.ops.fsgm.sgm_ru.default._schema).split("(", 1)[1]
    assert sgm_schema.split("(", 1)[1] == u8.replace("Tensor guide, ", "Tensor guide, float scale, float offset, ").replace(
        "SymInt return_sum)", "SymInt return_sum, bool runner_up, bool exact)")
    for name in ("sgm_float", "sgm2d_float", "sgm_f32"):
        assert not hasattr(torch.ops.fsgm, name)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_fake_outputs(dtype):
    ops = _torch_ops()
    from torch._subclasses.fake_tensor import FakeTensorMode
    u32, f64, dt = torch.uint32, torch.float64, getattr(torch, dtype)
    with FakeTensorMode():
        Cv = torch.empty((3, 16, 9, 33), dtype=dt, device="cuda")
        r = ops.sgm_float(Cv, 0.5, 3.0, 7, 100, paths=8, return_sum=True, return_status=True)
        assert [(tuple(t.shape), t.dtype) for t in r] == [((3, 9, 33), u32)] * 2 + [((3, 9, 33, 16), u32), ((), torch.int32)]
        r = ops.sgm_float(Cv[0], -2.0, runner_up=True)
        assert [(tuple(t.shape), t.dtype) for t in r] == [((9, 33), u32)] * 3
        r = ops.sgm_float(Cv.permute(0, 2, 3, 1).contiguous(), 1.0, layout="hwd", arith="exact")
        assert [(tuple(t.shape), t.dtype) for t in r] == [((3, 9, 33), u32)] * 2
        costs = torch.empty((2, 15, 9, 33), dtype=dt, device="cuda")
        r = ops.sgm2d_float(costs, 1, 2, 0.25, 1.0, layout="dhw_yx", runner_up=True, arith="exact", return_flow=True, return_sum=True,
                            return_status=True)
        assert [(tuple(t.shape), t.dtype) for t in r] == ([((2, 9, 33), u32)] * 3 + [((2, 2, 9, 33), f64)] * 2
                                                          + [((2, 9, 33, 15), u32), ((), torch.int32)])
        r = ops.sgm2d_float(costs[1], 1, 2, 4.0)
        assert [(tuple(t.shape), t.dtype) for t in r] == [((9, 33), u32)] * 2 + [((2, 9, 33), f64)]
        # the raw op: minC2 is the empty placeholder without runner_up
        empty = torch.empty((0,), dtype=torch.uint8, device="cuda")
        out = torch.ops.fsgm_float.sgm(Cv, empty, 1.0, 0.0, 7, 100, 4, 1, 255, 0, 0, 1, 0, False, False)
        assert [tuple(t.shape) for t in out] == [(3, 9, 33), (3, 9, 33), (0,), (0,), ()]


def test_torch_wrappers_type_errors():
    ops = _torch_ops()
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for dt in (torch.uint8, torch.float64, torch.int32):
            with pytest.raises(TypeError, match="torch.float32, torch.float16, torch.bfloat16"):
                ops.sgm_float(torch.empty((16, 9, 33), dtype=dt, device="cuda"), 1.0)
            with pytest.raises(TypeError, match="torch.float32, torch.float16, torch.bfloat16"):
                ops.sgm2d_float(torch.empty((9, 9, 33), dtype=dt, device="cuda"), 1, 1, 1.0)
        Cv = torch.empty((16, 9, 33), dtype=torch.float16, device="cuda")
        with pytest.raises(TypeError, match="GPU"):
            ops.sgm_float(torch.empty((16, 9, 33), dtype=torch.float16, device="cpu"), 1.0)
        with pytest.raises(TypeError, match="torch.Tensor"):
            ops.sgm_float(np.zeros((16, 9, 33), np.float32), 1.0)
        with pytest.raises(TypeError, match="guide must be torch.uint8"):
            ops.sgm_float(Cv, 1.0, guide=torch.empty((9, 33), dtype=torch.float16, device="cuda"), adaptive_p2=1)
        with pytest.raises(ValueError, match="runner"):
            ops.sgm_float(Cv, 1.0, arith="exact", runner_up=True)
        with pytest.raises(ValueError, match="layout"):
            ops.sgm_float(Cv, 1.0, layout="yx")
        with pytest.raises(TypeError, match="contiguous"):
            ops.sgm2d_float(torch.empty((9, 33, 9), dtype=torch.float32, device="cuda").permute(2, 0, 1), 1, 1, 1.0)
        with pytest.raises(ValueError, match="candidates"):
            ops.sgm2d_float(torch.empty((8, 9, 33), dtype=torch.float32, device="cuda"), 1, 1, 1.0)


def test_the_u8_torch_wrappers_still_refuse_floats():
    ops = _torch_ops()
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            with pytest.raises(TypeError, match="C must be torch.uint8"):
                ops.sgm(torch.empty((16, 9, 33), dtype=dt, device="cuda"))
            with pytest.raises(TypeError, match="costs must be torch.uint8"):
                ops.sgm2d(torch.empty((9, 9, 33), dtype=dt, device="cuda"), 1, 1)


def test_plan_ingest_helpers_type_errors():
    ops = _torch_ops()
    from torch._subclasses.fake_tensor import FakeTensorMode

    class Plan:                          # (what the helpers read of a plan before they call the library)
        device, batch, H, W, D = 0, 2, 9, 33, 16

    with FakeTensorMode():
        with pytest.raises(TypeError, match="torch.float32, torch.float16, torch.bfloat16"):
            ops.ingest_cost_float(Plan(), torch.empty((2, 16, 9, 33), dtype=torch.uint8, device="cuda"), 1.0)
        with pytest.raises(TypeError, match="shape"):
            ops.ingest_cost_float(Plan(), torch.empty((2, 9, 33, 16), dtype=torch.float16, device="cuda"), 1.0)
        with pytest.raises(TypeError, match="torch.float32, torch.float16, torch.bfloat16"):
            ops.ingest_cost2d_float(Plan(), torch.empty((2, 16, 9, 33), dtype=torch.float64, device="cuda"), 1.0)
        with pytest.raises(TypeError, match="contiguous"):
            ops.ingest_cost2d_float(Plan(), torch.empty((2, 9, 33, 16), dtype=torch.float32, device="cuda").permute(0, 3, 1, 2), 1.0)
        with pytest.raises(TypeError, match="C must be torch.uint8"):
            ops.ingest_cost(Plan(), torch.empty((2, 16, 9, 33), dtype=torch.float32, device="cuda"))
