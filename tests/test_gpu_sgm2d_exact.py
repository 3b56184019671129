"""GPU tests of the 2-D matcher with exact path arithmetic: fsgm_sgm2d_batch_host_exact (fsgm_amd.sgm2d_batch(arith="exact")),
fsgm_sgm2d_device_exact (torch_ops.sgm2d(arith="exact")) and the plan switch fsgm_pyd_plan_set_exact against the int64 restatement
of tests/sgm2d_exact_restatement.py.  Every comparison is equality of every element of bestD, minC, mvSub, flow, S and, where
asked, minC2: no tolerance.  tests/test_sgm2d_exact_cpu.py proves on the CPU that the inputs of tests/sgm2d_exact_cases.py lie
where the exact sums differ from the mod-256 ones."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops, synth, sgm2d_batch, PydPlan  # noqa: E402  (torch first, then the library)
from fsgm_amd import _lib  # noqa: E402
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd.sgm2d import last_kernel  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import sgm2d_exact_cases as K  # noqa: E402
from tests import sgm2d_exact_restatement as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_INVALID = 1
NAMES = ("bestD", "minC", "mvSub", "flow", "S", "minC2")


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cases' arrays are read-only)


def _n(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _same(got, want, what, names=NAMES):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        g = _n(g)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype} {g.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _run(form, c, vols, hints, guides, arith="exact", runner_up=False, **kw):
    """(bestD, minC, mvSub, flow, S[, minC2]) of the host or the device form on the case's shape and switches"""
    src = K.as_layout(c.layout, vols, 2 * c.rX + 1, 2 * c.rY + 1)
    kw = dict(dict(layout=c.layout, diagonal=c.diagonal, total_pass=c.passes, adaptive_p2=c.adaptive, subpixel=c.subpixel,
                   return_flow=True, return_sum=True, arith=arith, runner_up=runner_up), **kw)
    if form == "host":
        out = sgm2d_batch(src, c.rX, c.rY, c.P1, c.P2, hints=hints, guide=guides, **kw)
    else:
        out = torch_ops.sgm2d(_t(src), c.rX, c.rY, c.P1, c.P2, hints=_t(hints), guide=_t(guides), check=True, **kw)
    return (out[0], out[1]) + tuple(out[3:]) + (out[2],) if runner_up else out


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_exact_against_the_restatement(gpu_lib, oracle, c, form):
    vols, hints, guides = K.inputs(c)
    _same(_run(form, c, vols, hints, guides), K.want(c)[:5], form, NAMES[:5])
    assert last_kernel() == "generic/exact"


# ---------------------------------------------------------------------------------------------- 2. inside the budget
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("rX,rY", [(4, 4), (6, 6)], ids=["rows-9x9", "compact-13x13"])
def test_inside_the_budget_exact_equals_plain(gpu_lib, rX, rY, form):
    """cmax + P2 + max(P1, P2) = 55 + 100 + 100 <= 255: no narrowing changes a value, the two doors give the same bits"""
    c = K.Case(21, 13, rX, rY, 3, 7, 100, "dhw_yx", "general", 1, 1, 2, 1, "random")
    vols, hints, guides = K.inputs(c)
    vols = np.minimum(vols, 55)
    plain = _run(form, c, vols, hints, guides, arith="wrap", cost_bound=55)
    assert last_kernel() in ("rows", "rows/wide", "generic")
    exact = _run(form, c, vols, hints, guides, cost_bound=55)
    assert last_kernel() == "generic/exact"
    _same(exact, tuple(_n(p) for p in plain), form, NAMES[:5])


# ---------------------------------------------------------------------------------------------- 3. the runner-up cost
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("c", [K.Case(21, 13, 4, 4, 3, 7, 100, "dhw", "general", 0, 1, 2, 1, "random"),        # <= 256 candidates: kept sums
                               K.Case(7, 5, 8, 8, 1, 20, 200, "hwd", "beyond", 1, 1, 2, 1, "random"),          # 289: summed again
                               K.Case(7, 5, 1, 1, 1, 255, 255, "dhw_yx", None, 0, 1, 2, 1, "random")],         # 3x3: NO_RUNNER_UP occurs
                         ids=K.case_id)
def test_runner_up(gpu_lib, oracle, c, form):
    vols, hints, guides = K.inputs(c)
    want = K.want(c)
    if 2 * c.rX + 1 == 3:
        assert (want[5] == X.NO_RUNNER_UP).any()
    _same(_run(form, c, vols, hints, guides, runner_up=True), want, form)
    assert last_kernel() == "generic/exact"
    _same(_run(form, c, vols, hints, guides), want[:5], form + " without minC2", NAMES[:5])


# ---------------------------------------------------------------------------------------------- 4. cache isolation
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("rX,rY", [(4, 4), (6, 6)], ids=["9x9", "13x13"])
def test_exact_and_plain_calls_of_one_shape_keep_their_own_plans(gpu_lib, oracle, rX, rY, form):
    """plain, exact, plain, exact with minC2, plain with minC2, exact: each reports its own kernel and its own results"""
    c = K.Case(21, 13, rX, rY, 1, 7, 100, "dhw", "general", 0, 1, 2, 1, "random")
    vols, hints, guides = K.inputs(c)
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    oS = pyoracle.pyd_aggregate(np.zeros((c.H, c.W), np.uint8), vols[0], hints[0], Sx, Sy, c.P1, c.P2, 1, 2, 0)
    obd, omc, oms = pyoracle.pyd_wta(oS, Sx, Sy, 1)
    want = K.want(c)
    assert not np.array_equal(oS, want[4][0])

    def plain(ru=False):
        got = _run(form, c, vols, hints, guides, arith="wrap", runner_up=ru)
        assert last_kernel() == "generic/wrap"
        for g, w, name in zip((got[0], got[1], got[2], got[4]), (obd, omc, oms, oS), ("bestD", "minC", "mvSub", "S")):
            np.testing.assert_array_equal(_n(g)[0], w, err_msg=f"plain {name}")
        if ru:
            np.testing.assert_array_equal(_n(got[5])[0], X.runner_up(oS, obd, Sx, Sy), err_msg="plain minC2")

    def exact(ru=False):
        _same(_run(form, c, vols, hints, guides, runner_up=ru), want if ru else want[:5], "exact", NAMES if ru else NAMES[:5])
        assert last_kernel() == "generic/exact"

    plain(), exact(), plain(), exact(True), plain(True), exact(), plain()


# ---------------------------------------------------------------------------------------------- 5. the bound
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_a_byte_above_cost_bound(gpu_lib, oracle, layout):
    """the host form refuses the volume; the device form saturates, raises the status word and runs the exact recurrence on
    the saturated volume -- with bound 99 and P2 = 100 still outside the budget, and still "generic/exact" inside it"""
    c = K.Case(21, 13, 4, 4, 3, 7, 100, layout, "general", 0, 1, 2, 1, "random")
    vols, hints, guides = K.inputs(c)
    src = K.as_layout(layout, vols, 9, 9)
    with pytest.raises(FsgmError) as e:
        sgm2d_batch(src, 4, 4, 7, 100, layout=layout, hints=hints, cost_bound=99, arith="exact")
    assert e.value.status == FSGM_ERR_INVALID and "cost_bound 99" in str(e.value)
    for bound in (99, 24):
        *got, st = torch_ops.sgm2d(_t(src), 4, 4, 7, 100, layout=layout, hints=_t(hints), cost_bound=bound, arith="exact", return_flow=True,
                                   return_sum=True, return_status=True)
        torch.cuda.synchronize()
        assert int(st.item()) == FSGM_ERR_INVALID and last_kernel() == "generic/exact"
        _same(got, K.want(c, bound)[:5], f"saturated at {bound}", NAMES[:5])
    *got, st = torch_ops.sgm2d(_t(src), 4, 4, 7, 100, layout=layout, hints=_t(hints), arith="exact", return_flow=True, return_sum=True,
                               return_status=True)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    _same(got, K.want(c)[:5], "bound 255", NAMES[:5])


def test_penalties_outside_0_255_are_refused_with_a_device(gpu_lib):
    vols = K.volumes(7, 5, 9, 1, 3)
    for P1, P2 in ((-1, 100), (7, 256)):
        for call in (lambda: sgm2d_batch(vols, 1, 1, P1, P2, layout="hwd", arith="exact"),
                     lambda: torch_ops.sgm2d(_t(vols), 1, 1, P1, P2, layout="hwd", arith="exact")):
            with pytest.raises(FsgmError) as e:
                call()
            assert e.value.status == FSGM_ERR_INVALID and "0..255" in str(e.value)


# ---------------------------------------------------------------------------------------------- 6. the plan switch
def _plan_outputs(plan, f=0):
    return plan.download(f) + (plan.download_sum(f),)


@pytest.mark.parametrize("rX,rY", [(2, 2), (6, 4)], ids=["rows-5x5", "compact-13x9"])
def test_plan_built_from_an_image_pair(gpu_lib, oracle, rX, rY):
    """census costs (<= 24) at P1 = 20, P2 = 200: the plain plan wraps, set_exact(1) gives the recurrence on the plan's own cost
    volume, a WTA alone right after a toggle is refused, set_exact(0) restores the plain outputs"""
    W, H, n = 24, 16, 2
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    pairs = [synth.image_pair(W, H, 8, seed=4 + f) for f in range(n)]
    mvs = [synth.hint_map(W + 2, H + 1, "general", seed=6 + f, amp=2.0) for f in range(n)]
    with PydPlan(W, H, W + 2, H + 1, rX, rY, 2, batch=n) as plan:
        for f in range(n):
            plan.upload(f, pairs[f][0], pairs[f][1], mvs[f])
        plan.set_params(20, 200, 1, 2, 0, 1)
        plan.run()
        plain = [_plan_outputs(plan, f) for f in range(n)]
        costs = [plan.download_cost(f) for f in range(n)]
        assert max(int(c.max()) for c in costs) <= 24
        for f in range(n):                                       # the plain plan is the mod-256 oracle
            oS = pyoracle.pyd_aggregate(pairs[f][0], costs[f], mvs[f], Sx, Sy, 20, 200, 1, 2, 0)
            np.testing.assert_array_equal(plain[f][3], oS)
        plan.set_exact(1)
        for stage_call in (lambda: plan.run(_lib.STAGE_WTA), lambda: plan.download_sum(0), lambda: plan.time(_lib.STAGE_WTA)):
            with pytest.raises(FsgmError) as e:                  # the path volumes still hold L
                stage_call()
            assert e.value.status == FSGM_ERR_INVALID and "toggled" in str(e.value)
        plan.run()
        for f in range(n):
            bd, mc, ms, _, S, _ = X.sgm2d(costs[f], rX, rY, 20, 200, mvs[f])
            # (census costs <= 24 keep every L of these small windows within a byte although 24 + 200 + 200 is outside the budget
            # formula: the sums may equal the plain ones; test_plan_with_uploaded_costs_up_to_255 is where the two must differ)
            _same(_plan_outputs(plan, f), (bd, mc, ms, S), f"exact frame {f}", ("bestD", "minC", "mvSub", "S"))
            np.testing.assert_array_equal(plan.download_cost(f), costs[f])
        plan.run(_lib.STAGE_WTA)                                 # a WTA alone on y volumes that an exact aggregation wrote: fine
        plan.set_runner_up(1)
        plan.run(_lib.STAGE_WTA)
        for f in range(n):
            bd, mc, ms, _, S, m2 = X.sgm2d(costs[f], rX, rY, 20, 200, mvs[f])
            _same(_plan_outputs(plan, f) + (plan.download_runner_up(f),), (bd, mc, ms, S, m2), f"exact + minC2 frame {f}",
                  ("bestD", "minC", "mvSub", "S", "minC2"))
        plan.set_runner_up(0)
        for bad in ((-1, 100), (20, 256)):                       # with the switch on the plan refuses what the kernels cannot hold
            with pytest.raises(FsgmError) as e:
                plan.set_params(*bad, 1, 2, 0, 1)
            assert e.value.status == FSGM_ERR_INVALID
        plan.set_exact(0)
        with pytest.raises(FsgmError) as e:                      # the path volumes hold y now
            plan.run(_lib.STAGE_WTA)
        assert e.value.status == FSGM_ERR_INVALID
        plan.set_exact(1)
        plan.run(_lib.STAGE_WTA)                                 # toggled back with no aggregation in between: the volumes fit again
        plan.set_exact(0)
        plan.run()
        for f in range(n):
            _same(_plan_outputs(plan, f), plain[f], f"plain again, frame {f}", ("bestD", "minC", "mvSub", "S"))
        plan.set_params(20, 300, 1, 2, 0, 1)                     # a plain plan takes any penalty, and then refuses the switch
        with pytest.raises(FsgmError) as e:
            plan.set_exact(1)
        assert e.value.status == FSGM_ERR_INVALID and "0..255" in str(e.value)
        plan.run()                                               # still plain


def test_plan_with_uploaded_costs_up_to_255(gpu_lib, oracle):
    """the switch on a plan whose volume came through upload_cost, adaptive P2 read from the plan's first image"""
    c = K.Case(21, 13, 2, 5, 1, 7, 100, "hwd", "general", 1, 1, 2, 1, "random")
    vols, hints, guides = K.inputs(c)
    mvH, mvW = hints.shape[-2:]
    with PydPlan(c.W, c.H, mvW, mvH, c.rX, c.rY, 2) as plan:
        plan.upload(0, guides[0], guides[0], hints[0])
        plan.upload_cost(0, vols[0])
        plan.set_params(c.P1, c.P2, 1, 2, 1, 1)
        plan.run(_lib.STAGE_AGGREGATE | _lib.STAGE_WTA)
        w = K.want(c)
        plainS = plan.download_sum(0)
        np.testing.assert_array_equal(plainS, pyoracle.pyd_aggregate(guides[0], vols[0], hints[0], 5, 11, c.P1, c.P2, 1, 2, 1))
        assert not np.array_equal(plainS, w[4][0]), "bytes up to 255 at P2 = 100: the plain plan wraps"
        plan.set_exact(1)
        plan.run(_lib.STAGE_AGGREGATE | _lib.STAGE_WTA)
        _same(_plan_outputs(plan), (w[0][0], w[1][0], w[2][0], w[4][0]), "uploaded", ("bestD", "minC", "mvSub", "S"))
