"""GPU tests of the 2-D matcher on caller-supplied cost volumes: the ingest kernels alone (every layout into the plan's padded
rows and back), then fsgm_sgm2d_batch_host and fsgm_sgm2d_device against the oracle's 2-D aggregation and WTA (pinned to the
reference's compiled code), bit for bit -- mvSub and flow included: they are f64 results of the same operations in the same order.

The yardstick is pyd_wta(pyd_aggregate(guide or zeros, min(C, cost_bound), hints or zeros, ...)) and, for the flow,
hints[:, :H, :W] + window offset + mvSub.

The channel-major ingest kernel's tile is 64 pixels x 64 bytes of the padded candidate index (fsgm_amd/csrc/sgm2d_ingest.hip);
the windows below give padded pixel sizes PS of 4, 24, 20, 108 (two tiles), 132, 117 (unpadded, odd) and 1023, the widths cross
1, 3, a tile, a tile + 1 and two tiles + 3."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, synth, sgm2d_batch, calc_pyd_cost_sgm, PydPlan  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd.sgm2d import last_kernel  # noqa: E402
from oracle import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_INVALID = 1
LAYOUTS = ("hwd", "dhw", "dhw_yx")
# (halfX, halfY): 1x1; 3x5 (RS 8, padded); 5x3 (RS 4); 9x9 (81 candidates cross a 64-byte tile); 11x11 (the largest rows layout);
# 13x9 (unpadded, PS 117); 31x33 (1023 candidates)
WINDOWS = [(0, 0), (1, 2), (2, 1), (4, 4), (5, 5), (6, 4), (15, 16)]
ROWS_WINDOWS = [w for w in WINDOWS if 2 * w[0] + 1 <= 11 and 2 * w[1] + 1 <= 11]
PENALTIES = [(6, 32, 24), (6, 32, 255)]      # (P1, P2, cost_bound = the volume's largest cost): no-wrap, and wrapping


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _volumes(W, H, D, n, seed, cmax):
    """(n, H, W, D) uint8 in reference order, every frame its own draw, the bound reached"""
    v = np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])
    v[-1, -1, -1, -1] = cmax
    return v


def _as(layout, vols, Sx, Sy):
    """the same volumes as the caller of that layout holds them"""
    n, H, W, D = vols.shape
    if layout == "hwd":
        return vols
    if layout == "dhw":
        return np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(vols.reshape(n, H, W, Sx, Sy).transpose(0, 4, 3, 1, 2).reshape(n, D, H, W))


def _hints(kind, n, W, H, seed):
    if kind is None:
        return None
    mvW, mvH = (W + 3, H + 3) if kind == "larger" else (W, H)
    return np.stack([synth.hint_map(mvW, mvH, "general", seed=seed + 5 * f, amp=3.0) for f in range(n)])


@functools.lru_cache(maxsize=None)
def _oracle_cached(key, rX, rY, P1, P2, bound, diag, passes, adaptive, sub):
    vols, hints, guide = _INPUTS[key]
    n, H, W, D = vols.shape
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    out = []
    for f in range(n):
        mv = np.zeros((2, H, W)) if hints is None else hints[f]
        I1 = np.zeros((H, W), np.uint8) if guide is None else guide[f]
        S = pyoracle.pyd_aggregate(I1, np.minimum(vols[f], bound), mv, Sx, Sy, P1, P2, diag, passes, adaptive)
        bd, mc, ms = pyoracle.pyd_wta(S, Sx, Sy, sub)
        off = np.stack([bd // Sy, bd % Sy]).astype(np.float64) - np.array([rX, rY], np.float64)[:, None, None]
        flow = mv[:, :H, :W] + off + ms
        out.append((bd, mc, ms, flow, S))
    return tuple(np.stack([o[k] for o in out]) for k in range(5))


_INPUTS = {}


def _want(vols, hints, guide, rX, rY, P1, P2, bound, diag=1, passes=2, adaptive=0, sub=1):
    """(bestD, minC, mvSub, flow, S) of the oracle for every frame, computed once per distinct input and left unchanged"""
    key = tuple((a.shape, hash(a.tobytes())) if a is not None else None for a in (vols, hints, guide))
    _INPUTS.setdefault(key, (vols, hints, guide))
    return _oracle_cached(key, rX, rY, P1, P2, bound, diag, passes, adaptive, sub)


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("bestD", "minC", "mvSub", "flow", "S")):
        np.testing.assert_array_equal(_n(g), w, err_msg=f"{what}: {name}")


def _run(form, layout, vols, rX, rY, P1, P2, hints=None, guide=None, **kw):
    """(bestD, minC, mvSub, flow, S) of the host or the device form"""
    src = _as(layout, vols, 2 * rX + 1, 2 * rY + 1)
    if form == "host":
        return sgm2d_batch(src, rX, rY, P1, P2, layout=layout, hints=hints, guide=guide, return_flow=True, return_sum=True, **kw)
    return torch_ops.sgm2d(_t(src), rX, rY, P1, P2, layout=layout, hints=None if hints is None else _t(hints),
                           guide=None if guide is None else _t(guide), return_flow=True, return_sum=True, check=True, **kw)


@pytest.fixture(scope="module")
def rows_available(gpu_lib):
    """Whether plans on this device hold the row-packed kernels' descriptors: fsgm_pyd_plan_create drops them when the device's
    once-a-device self-test of the packed 3-input minima fails (tests/test_gpu_pyd_windows.py), and the generic kernels then run
    every case -- equal to the oracle all the same.  Asked with the smallest call that would take them."""
    sgm2d_batch(np.zeros((9, 2, 3), np.uint8), 1, 1, 6, 32, layout="dhw", cost_bound=24)
    return last_kernel().startswith("rows")


def _expect_kernel(rows_available, rX, rY, n, W, H, bound, P1=6, P2=32):
    """pyd_enqueue's choice, restated: the declared bound decides between wrapping and not, the window and the plan's
    descriptors between row-packed and generic, the batch and the frame's shape between the two row-packed mappings."""
    if bound + P2 + max(P1, P2) > 255:
        return "generic/wrap"
    if (rX, rY) in ROWS_WINDOWS and rows_available:
        return "rows/wide" if n <= 2 and W > H else "rows"
    return "generic"


# ---------------------------------------------------------------------------------------------- 1. the ingest kernels alone
def _round_trip(W, H, rX, rY, n, layout, bound=255):
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    vols = _volumes(W, H, Sx * Sy, n, seed=W + 7 * H + Sx, cmax=255)
    with PydPlan(W, H, W, H, rX, rY, 0, batch=n) as plan:
        st = plan.ingest_cost(_t(_as(layout, vols, Sx, Sy)), layout=layout, cost_bound=bound, return_status=True)
        for f in range(n):
            np.testing.assert_array_equal(plan.download_cost(f), np.minimum(vols[f], bound), err_msg=f"{layout} {W}x{H} {Sx}x{Sy} frame {f}")
        assert int(st.item()) == (0 if bound == 255 else FSGM_ERR_INVALID)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rX,rY", WINDOWS)
def test_layout_round_trip(gpu_lib, rX, rY, layout):
    W, H = (9, 7) if (rX, rY) == (15, 16) else (67, 5)
    _round_trip(W, H, rX, rY, 2, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(1, 1), (3, 1), (64, 2), (65, 3), (131, 2)])
def test_layout_round_trip_image_sizes(gpu_lib, W, H, layout):
    _round_trip(W, H, 1, 2, 2, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rX,rY,bound", [(1, 2, 100), (4, 4, 1), (6, 4, 254), (0, 0, 127)])
def test_ingest_saturates_at_the_bound(gpu_lib, rX, rY, bound, layout):
    _round_trip(67, 5, rX, rY, 3, layout, bound)


# ---------------------------------------------------------------------------------------------- 2. the full call against the oracle
@pytest.mark.parametrize("P1,P2,bound", PENALTIES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rX,rY", WINDOWS)
def test_results_against_the_oracle(gpu_lib, oracle, rows_available, rX, rY, n, P1, P2, bound):
    """every layout through the device form, one of them through the host form too; hints on a map larger than the image"""
    W, H, D = 40, 12, (2 * rX + 1) * (2 * rY + 1)
    vols = _volumes(W, H, D, n, seed=3 + rX, cmax=bound)
    hints = _hints("larger", n, W, H, seed=40 + rY)
    assert hints.shape == (n, 2, 15, 43)
    want = _want(vols, hints, None, rX, rY, P1, P2, bound)
    kernel = _expect_kernel(rows_available, rX, rY, n, W, H, bound)
    for layout in LAYOUTS:
        _same(_run("device", layout, vols, rX, rY, P1, P2, hints, cost_bound=bound), want, f"device {layout}")
        assert last_kernel() == kernel
    host_layout = LAYOUTS[(rX + n) % 3]
    _same(_run("host", host_layout, vols, rX, rY, P1, P2, hints, cost_bound=bound), want, f"host {host_layout}")
    assert last_kernel() == kernel


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("diag", [0, 1])
@pytest.mark.parametrize("rX,rY,bound", [(4, 4, 24), (4, 4, 255), (6, 4, 24)])
def test_path_sets_passes_subpixel_and_hints(gpu_lib, oracle, rX, rY, bound, diag, passes, sub):
    """hints NULL (plain sgm2d), fractional on a map of the image's size, and on a larger map; both forms"""
    W, H, n, D = 40, 12, 1, (2 * rX + 1) * (2 * rY + 1)
    vols = _volumes(W, H, D, n, seed=17, cmax=bound)
    kw = dict(cost_bound=bound, diagonal=diag, total_pass=passes, subpixel=sub)
    for i, kind in enumerate((None, "same", "larger")):
        hints = _hints(kind, n, W, H, seed=50)
        want = _want(vols, hints, None, rX, rY, 6, 32, bound, diag, passes, 0, sub)
        if not sub:
            assert not want[2].any()
        _same(_run("device", LAYOUTS[(i + diag) % 3], vols, rX, rY, 6, 32, hints, **kw), want, f"device hints {kind}")
        _same(_run("host", LAYOUTS[(i + passes) % 3], vols, rX, rY, 6, 32, hints, **kw), want, f"host hints {kind}")


def test_single_volume_without_the_batch_axis(gpu_lib, oracle):
    W, H, rX, rY = 40, 12, 1, 2
    vols = _volumes(W, H, 15, 1, seed=21, cmax=24)
    want = tuple(w[0] for w in _want(vols, None, None, rX, rY, 6, 32, 24))
    got = sgm2d_batch(_as("dhw_yx", vols, 3, 5)[0], rX, rY, layout="dhw_yx", cost_bound=24, return_flow=True, return_sum=True)
    _same(got, want, "host")
    got = torch_ops.sgm2d(_t(_as("dhw_yx", vols, 3, 5)[0]), rX, rY, layout="dhw_yx", cost_bound=24, return_flow=True, return_sum=True)
    _same(got, want, "device")
    _same(sgm2d_batch(vols[0], rX, rY, layout="hwd", cost_bound=24), want[:3], "no optional outputs")


@pytest.mark.parametrize("rX,rY", [(2, 2), (6, 4)])
@pytest.mark.parametrize("n", [1, 3])
def test_adaptive_p2(gpu_lib, oracle, n, rX, rY):
    """a guide with an intensity step above 50 down the middle: P2 / 8 across it (calc_pyd_cost_sgm.cpp:91-95)"""
    W, H, D = 40, 12, (2 * rX + 1) * (2 * rY + 1)
    vols = _volumes(W, H, D, n, seed=23, cmax=24)
    hints = _hints("same", n, W, H, seed=60)
    guide = np.stack([synth.image_pair(W, H, 16, seed=30 + f)[0] // 2 for f in range(n)])
    guide[:, :, W // 2:] += 120
    assert (np.abs(guide[:, :, W // 2].astype(int) - guide[:, :, W // 2 - 1].astype(int)) > 50).all()
    want = _want(vols, hints, guide, rX, rY, 6, 32, 24, adaptive=1)
    plain = _want(vols, hints, None, rX, rY, 6, 32, 24, adaptive=0)
    assert not np.array_equal(want[4], plain[4]), "the edge must matter"
    for form, layout in (("host", "hwd"), ("device", "dhw"), ("host", "dhw_yx")):
        _same(_run(form, layout, vols, rX, rY, 6, 32, hints, guide, cost_bound=24, adaptive_p2=1), want, f"{form} {layout}")
    _same(_run("device", "dhw", vols, rX, rY, 6, 32, hints, guide, cost_bound=24), plain, "the guide is not read without adaptive_p2")
    for call in (lambda: sgm2d_batch(vols, rX, rY, layout="hwd", adaptive_p2=1),
                 lambda: torch_ops.sgm2d(_t(vols), rX, rY, layout="hwd", adaptive_p2=1)):
        with pytest.raises(FsgmError) as e:
            call()
        assert e.value.status == FSGM_ERR_INVALID


# ---------------------------------------------------------------------------------------------- 3. the bound
@pytest.mark.parametrize("rX,rY", [(4, 4), (6, 4)])
def test_saturation(gpu_lib, oracle, rows_available, rX, rY):
    W, H, n, D = 40, 12, 3, (2 * rX + 1) * (2 * rY + 1)
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    clean = _volumes(W, H, D, n, seed=8, cmax=24)
    vols = clean.copy()
    vols[0, 0, 0, 0] = vols[1, 4, 17, 9] = vols[2, H - 1, W - 1, D - 1] = 200
    want = _want(np.minimum(vols, 24), None, None, rX, rY, 6, 32, 24)
    for layout in LAYOUTS:
        src = _as(layout, vols, Sx, Sy)
        # the host form refuses, the outputs untouched
        with pytest.raises(FsgmError) as e:
            sgm2d_batch(src, rX, rY, layout=layout, cost_bound=24)
        assert e.value.status == FSGM_ERR_INVALID and "cost_bound 24" in str(e.value)
        # the device form saturates and says so
        *got, st = torch_ops.sgm2d(_t(src), rX, rY, layout=layout, cost_bound=24, return_flow=True, return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == FSGM_ERR_INVALID and last_kernel() == _expect_kernel(rows_available, rX, rY, n, W, H, 24)
        _same(got, want, f"saturated {layout}")
        with pytest.raises(FsgmError) as e:
            torch_ops.sgm2d(_t(src), rX, rY, layout=layout, cost_bound=24, check=True)
        assert e.value.status == FSGM_ERR_INVALID
        # a clean volume, and the same volume under the full bound: status 0
        *got, st = torch_ops.sgm2d(_t(_as(layout, clean, Sx, Sy)), rX, rY, layout=layout, cost_bound=24, return_flow=True, return_sum=True,
                                   return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        _same(got, _want(clean, None, None, rX, rY, 6, 32, 24), f"clean {layout}")
        *got, st = torch_ops.sgm2d(_t(src), rX, rY, layout=layout, cost_bound=255, return_flow=True, return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and last_kernel() == "generic/wrap"
        _same(got, _want(vols, None, None, rX, rY, 6, 32, 255), f"bound 255 {layout}")


def test_host_form_leaves_the_outputs_of_a_refused_volume_untouched(gpu_lib):
    from fsgm_amd import _lib
    from fsgm_amd.sgm2d import _bind, params
    import ctypes as C
    lib = _bind(_lib.load())
    W, H, rX, rY = 40, 12, 4, 4
    vols = _volumes(W, H, 81, 1, seed=8, cmax=24)
    vols[0, 5, 6, 7] = 25
    bestD, minC = np.full((1, H, W), 0xDEADBEEF, np.uint32), np.full((1, H, W), 0xDEADBEEF, np.uint32)
    mvSub, flow = np.full((1, 2, H, W), -7.0), np.full((1, 2, H, W), -7.0)
    prm = params(lib, layout="hwd", cost_bound=24)
    p = _lib.ptr
    st = lib.fsgm_sgm2d_batch_host(1, p(vols), W, H, rX, rY, 6, 32, C.byref(prm), None, 0, 0, None, p(bestD), p(minC), p(mvSub), p(flow), None)
    assert st == FSGM_ERR_INVALID
    assert (bestD == 0xDEADBEEF).all() and (minC == 0xDEADBEEF).all() and (mvSub == -7.0).all() and (flow == -7.0).all()


# ---------------------------------------------------------------------------------------------- 4. the existing matcher
@pytest.mark.parametrize("rX,rY", [(2, 2), (6, 4)])
def test_agreement_with_calc_pyd_cost_sgm(gpu_lib, rX, rY):
    """calc_pyd_cost_sgm's own cost volume, fed back with the same hints: the MEX's outputs"""
    W, H = 40, 12
    I1, I2 = synth.image_pair(W, H, 8, seed=4)
    mv = synth.hint_map(W + 2, H + 1, "general", seed=6, amp=2.0)
    bd, mc, ms, Cv, S = calc_pyd_cost_sgm(I1, I2, mv, rX, rY, 2, 1, 6, 32, 1, 2, 0, return_volumes=True)
    assert Cv.max() <= 24
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    for layout in LAYOUTS:
        got = sgm2d_batch(_as(layout, Cv[None], Sx, Sy)[0], rX, rY, 6, 32, layout=layout, hints=mv, cost_bound=24, return_sum=True)
        for g, w, name in zip(got, (bd, mc, ms, S), ("bestD", "minC", "mvSub", "S")):
            np.testing.assert_array_equal(g, w, err_msg=f"{layout} {name}")


# ---------------------------------------------------------------------------------------------- 5. plan reuse
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plan_reuse_leaves_no_stale_bytes(gpu_lib, oracle, form, layout):
    """two calls of one shape on one cached plan: all-255 bytes, then an ordinary volume -- a 3 x 5 window, whose rows of 5
    candidates lie 8 bytes apart; then a call without hints behind one with hints"""
    W, H, n, rX, rY = 40, 12, 3, 1, 2
    full = np.full((n, H, W, 15), 255, np.uint8)
    vols = _volumes(W, H, 15, n, seed=31, cmax=24)
    _same(_run(form, layout, full, rX, rY, 6, 32, cost_bound=255), _want(full, None, None, rX, rY, 6, 32, 255), "all 255")
    _same(_run(form, layout, vols, rX, rY, 6, 32, cost_bound=255), _want(vols, None, None, rX, rY, 6, 32, 255), "after all 255, wrapping")
    _same(_run(form, layout, full, rX, rY, 6, 32, cost_bound=255), _want(full, None, None, rX, rY, 6, 32, 255), "all 255 again")
    _same(_run(form, layout, vols, rX, rY, 6, 32, cost_bound=24), _want(vols, None, None, rX, rY, 6, 32, 24), "after all 255, rows")
    hints = _hints("same", n, W, H, seed=70)
    _same(_run(form, layout, vols, rX, rY, 6, 32, hints, cost_bound=24), _want(vols, hints, None, rX, rY, 6, 32, 24), "with hints")
    _same(_run(form, layout, vols, rX, rY, 6, 32, cost_bound=24), _want(vols, None, None, rX, rY, 6, 32, 24), "without, after with")
